"""Collated reduce on the GPU (mz_gpu_collation_*): COUNT/SUM and MIN/MAX
maintained behind one operator, against a naive full recompute.

The oracle has no collation, so the reference lives here: the model is
key -> multiset of val rows; after each step the stitched row of every live
key is computed from scratch and the expected corrections are the
difference from the previous step's rows. Everything compares bit-exact as
sorted lists of (key, val bytes, time, diff).

Input rows are 24 bytes: a = i64 @0, b = i64 @8, c = i32 @16, 4 pad bytes.
"""
import functools
import struct

import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

pytestmark = pytest.mark.gpu

ROW = np.dtype([("a", "<i8"), ("b", "<i8"), ("c", "<i4"), ("pad", "<i4")])
SLOT = abi.AGG_SLOT_BYTES


def agg(func, off=0, width=8, is_float=0):
    return abi.Aggregate(func=func, off=off, width=width, is_float=is_float,
                         nullable=0)


COUNT = agg(abi.MZ_AGG_COUNT)
SUM_A = agg(abi.MZ_AGG_SUM_I64, 0)
MIN_B = agg(abi.AGG_MIN_I64, 8)
MAX_C = agg(abi.AGG_MAX_I64, 16, 4)
DEFAULT_AGGS = (COUNT, SUM_A, MIN_B, MAX_C)
BUCKETS = (16, 1)


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


def rows(a, b, c):
    a = np.asarray(a, np.int64)
    r = np.zeros(len(a), ROW)
    r["a"], r["b"], r["c"] = a, b, c
    return r


def updates(keys, vals, diffs, t, upper=None):
    keys = np.ascontiguousarray(keys, np.int64)
    n = len(diffs)
    return abi.make_updates(keys.ravel(), vals.view(np.uint8).ravel(),
                            np.full(n, t, np.uint64),
                            np.asarray(diffs, np.int64), t,
                            t + 1 if upper is None else upper)


def out_rows(out, kw, vb):
    keys, vals, times, diffs = out
    return sorted(
        (tuple(int(x) for x in keys[i * kw:(i + 1) * kw]),
         vals[i * vb:(i + 1) * vb].tobytes(), int(times[i]), int(diffs[i]))
        for i in range(len(times)))


def assert_canonical_keys(out, kw):
    """Consolidated output comes in canonical order: keys ascending as
    signed tuples."""
    k = [tuple(int(x) for x in out[0][i * kw:(i + 1) * kw])
         for i in range(len(out[2]))]
    assert k == sorted(k)


# ------------------------------------------------------------ naive model
def datum(v, a):
    return int.from_bytes(v[a.off:a.off + a.width], "little", signed=True)


def slot(a, counter):
    s = bytearray(SLOT)
    if a.func == abi.MZ_AGG_COUNT:
        s[8:16] = struct.pack("<q", sum(counter.values()))
    elif a.func == abi.MZ_AGG_SUM_I64:
        tot = sum(datum(v, a) * c for v, c in counter.items())
        s[8:24] = (tot % (1 << 128)).to_bytes(16, "little")
    elif a.func == abi.MZ_AGG_SUM_F64:
        # inputs are multiples of 0.5 below 2^20: exact in the engine's
        # 24-fractional-bit fixed point and in this float sum
        tot = sum(struct.unpack_from("<d", v, a.off)[0] * c
                  for v, c in counter.items())
        s[8:16] = struct.pack("<d", tot)
    else:
        vals = [datum(v, a) for v in counter]
        m = max(vals) if a.func == abi.AGG_MAX_I64 else min(vals)
        s[8:16] = struct.pack("<q", m)
    return bytes(s)


class Naive:
    def __init__(self, aggs, kw):
        self.aggs, self.kw = list(aggs), kw
        self.model = {}   # key tuple -> {val bytes: count}
        self.rows = {}    # key tuple -> stitched row of the last step

    def step(self, keys, vals, diffs, t):
        keys = np.asarray(keys, np.int64).reshape(-1, self.kw)
        raw = vals.view(np.uint8).reshape(len(diffs), -1)
        for k, v, d in zip(keys, raw, diffs):
            k, v = tuple(int(x) for x in k), v.tobytes()
            cnt = self.model.setdefault(k, {})
            cnt[v] = cnt.get(v, 0) + int(d)
            if cnt[v] == 0:
                del cnt[v]
            if not cnt:
                del self.model[k]
        new = {k: b"".join(slot(a, cnt) for a in self.aggs)
               for k, cnt in self.model.items()}
        exp = []
        for k in set(new) | set(self.rows):
            o, n = self.rows.get(k), new.get(k)
            if o == n:
                continue
            if o is not None:
                exp.append((k, o, t, -1))
            if n is not None:
                exp.append((k, n, t, 1))
        self.rows = new
        return sorted(exp)


class Rig:
    """A collated operator and its naive model, stepped together."""

    def __init__(self, g, aggs=DEFAULT_AGGS, kw=1, buckets=BUCKETS):
        self.g, self.kw = g, kw
        self.aggs = list(aggs)
        self.vb = SLOT * len(self.aggs)
        spec = abi.collation_spec(self.aggs, abi.schema(kw, ROW.itemsize),
                                  buckets=buckets)
        self.op = g.collation_create(spec)
        self.naive = Naive(self.aggs, kw)
        self.t = 0

    def step(self, keys, vals, diffs):
        t = self.t
        self.t += 1
        out = self.g.collation_push(self.op, updates(keys, vals, diffs, t))
        got = out_rows(out, self.kw, self.vb)
        want = self.naive.step(keys, vals, diffs, t)
        assert got == want, f"step {t}"
        assert_canonical_keys(out, self.kw)
        return got

    def drop(self):
        self.g.collation_drop(self.op)


def key_words(k, kw):
    """kw = 2 spreads the ids over both words, negatives included."""
    k = np.asarray(k, np.int64)
    if kw == 1:
        return (k - 50).reshape(-1, 1)
    return np.stack([k % 7 - 3, k // 7 - 5], axis=1)


@functools.lru_cache(maxsize=None)
def churn_stream(kw, seed=11, steps=6, n=2000, nkeys=100):
    """tests/test_minmax.py's churn: 40 % of the rows retract a row that is
    present. Returns per step (keys[n,kw], rows[n], diffs[n])."""
    rng = np.random.default_rng(seed)
    present, out = [], []
    for _ in range(steps):
        ks, rs, ds = [], [], []
        for _ in range(n):
            if present and rng.random() < 0.4:
                k, r = present.pop(int(rng.integers(0, len(present))))
                d = -1
            else:
                k = int(rng.integers(0, nkeys))
                r = (int(rng.integers(-1000, 1000)),
                     int(rng.integers(-50, 50)),
                     int(rng.integers(-50, 50)))
                d = 1
                present.append((k, r))
            ks.append(k)
            rs.append(r)
            ds.append(d)
        a, b, c = (np.array(x) for x in zip(*rs))
        out.append((key_words(ks, kw), rows(a, b, c),
                    np.array(ds, np.int64)))
    return out


# 1 --------------------------------------------------------- churn parity
@pytest.mark.parametrize("kw", [1, 2])
def test_churn_parity(g, kw):
    rig = Rig(g, kw=kw)
    for keys, vals, diffs in churn_stream(kw):
        rig.step(keys, vals, diffs)
    rig.drop()


# 2 ------------------------------------------------- only one part changes
def test_only_one_part_changes(g):
    rig = Rig(g)
    nk = 10
    k3 = np.repeat(np.arange(nk), 3)
    rig.step(k3.reshape(-1, 1),
             rows(np.tile([1, 2, 3], nk), np.tile([10, 20, 30], nk),
                  np.tile([10, 20, 30], nk)), np.ones(3 * nk, np.int64))
    # b and c strictly inside [min, max]: COUNT and SUM move, the MIN and
    # MAX slots are carried from the stitch state
    got = rig.step(np.arange(5).reshape(-1, 1),
                   rows([5] * 5, [15] * 5, [15] * 5), np.ones(5, np.int64))
    assert len(got) == 10
    for _, v, _, d in got:
        assert struct.unpack_from("<q", v, 2 * SLOT + 8)[0] == 10
        assert struct.unpack_from("<q", v, 3 * SLOT + 8)[0] == 30
        assert struct.unpack_from("<q", v, 8)[0] == (3 if d < 0 else 4)
    # converse: swap (1, 10, 10) for (1, 5, 10) — only MIN changes
    ks = np.repeat(np.arange(5, 10), 2).reshape(-1, 1)
    got = rig.step(ks, rows([1, 1] * 5, [10, 5] * 5, [10, 10] * 5),
                   np.tile([-1, 1], 5))
    assert len(got) == 10
    by_key = {}
    for k, v, _, d in got:
        by_key.setdefault(k, {})[d] = v
    for k, pair in by_key.items():
        old, new = pair[-1], pair[1]
        assert old[:2 * SLOT] == new[:2 * SLOT]      # COUNT, SUM slots
        assert old[3 * SLOT:] == new[3 * SLOT:]      # MAX slot
        assert struct.unpack_from("<q", old, 2 * SLOT + 8)[0] == 10
        assert struct.unpack_from("<q", new, 2 * SLOT + 8)[0] == 5
    # nil net effect on keys 0 and 1 (an insert+retract of one row; a swap
    # of an interior row for another with the same a), a real change on 2
    got = rig.step(
        np.array([0, 0, 1, 1, 2]).reshape(-1, 1),
        rows([7, 7, 2, 2, 9], [7, 7, 20, 25, 0], [7, 7, 20, 25, 0]),
        np.array([1, -1, -1, 1, 1]))
    assert sorted({k for k, _, _, _ in got}) == [(2,)]
    # a step that is nil for every key emits nothing at all
    got = rig.step(np.array([3, 3]).reshape(-1, 1),
                   rows([4, 4], [12, 12], [12, 12]), np.array([1, -1]))
    assert got == []
    rig.drop()


# 3 ------------------------------------------------ group death and rebirth
def test_group_death_and_rebirth(g):
    rig = Rig(g)
    nk = 20
    k3 = np.repeat(np.arange(nk), 3)
    a = np.arange(3 * nk)
    first = rows(a, a * 3 - 40, 50 - a)
    rig.step(k3.reshape(-1, 1), first, np.ones(3 * nk, np.int64))
    dead = k3 < 8
    got = rig.step(k3[dead].reshape(-1, 1), first[dead],
                   -np.ones(dead.sum(), np.int64))
    assert [(k, d) for k, _, _, d in got] == [((k,), -1) for k in range(8)]
    rig.step(np.array([[10]]), rows([1], [1], [1]), np.array([1]))
    rig.step(np.array([[11]]), rows([2], [2], [2]), np.array([1]))
    got = rig.step(np.arange(8).reshape(-1, 1),
                   rows(np.arange(8) + 100, np.arange(8) - 7,
                        np.arange(8) * 2), np.ones(8, np.int64))
    assert [(k, d) for k, _, _, d in got] == [((k,), 1) for k in range(8)]
    rig.drop()


# 4 ------------------------------------ wave / grid edges of k_collate_apply
def one_row_expected(a, b, c):
    """Stitched DEFAULT_AGGS rows of groups holding exactly one row."""
    n = len(a)
    out = np.zeros((n, 4 * SLOT), np.uint8)
    i64 = lambda x: np.ascontiguousarray(x, np.int64).view(np.uint8) \
        .reshape(n, 8)
    out[:, 8:16] = i64(np.ones(n))
    out[:, SLOT + 8:SLOT + 16] = i64(a)
    out[:, SLOT + 16:SLOT + 24] = i64(np.asarray(a) >> 63)  # i128 sign
    out[:, 2 * SLOT + 8:2 * SLOT + 16] = i64(b)
    out[:, 3 * SLOT + 8:3 * SLOT + 16] = i64(c)
    return out


def assert_one_row_step(out, keys, vals, diffs, t):
    """Vectorised parity for steps with at most one -1 and one +1 row per
    key: order both sides by (key, diff)."""
    gk, gv, gt, gd = out
    assert len(gt) == len(keys)
    o = np.lexsort((gd, gk))
    e = np.lexsort((diffs, keys))
    np.testing.assert_array_equal(gk[o], keys[e])
    np.testing.assert_array_equal(gd[o], diffs[e])
    np.testing.assert_array_equal(gv.reshape(len(gt), -1)[o], vals[e])
    assert (gt == t).all()
    assert (np.diff(gk) >= 0).all()  # canonical key order


def fresh_rows(rng, n):
    return rows(rng.integers(-1000, 1000, n),
                rng.integers(-(1 << 40), 1 << 40, n),
                rng.integers(-(1 << 31), 1 << 31, n))


def push_default(g, op, keys, r, diffs, t):
    return g.collation_push(op, updates(keys, r, diffs, t))


def test_apply_wave_edges(g):
    rng = np.random.default_rng(4)
    op = g.collation_create(abi.collation_spec(
        DEFAULT_AGGS, abi.schema(1, ROW.itemsize), buckets=BUCKETS))
    base = 0
    for t, m in enumerate([1, 63, 64, 65, 257]):
        keys = rng.permutation(np.arange(base, base + m)).astype(np.int64)
        base += m
        r = fresh_rows(rng, m)
        out = push_default(g, op, keys, r, np.ones(m, np.int64), t)
        assert_one_row_step(out, keys, one_row_expected(r["a"], r["b"],
                                                        r["c"]),
                            np.ones(m, np.int64), t)
    g.collation_drop(op)


def test_apply_second_grid_iteration(g):
    # the launch caps at 2048 blocks of 256 threads: this is the first
    # group count with a second grid-stride iteration and a partial wave
    m = 2048 * 256 + 65
    rng = np.random.default_rng(5)
    op = g.collation_create(abi.collation_spec(
        DEFAULT_AGGS, abi.schema(1, ROW.itemsize), buckets=BUCKETS))
    keys = rng.permutation(m).astype(np.int64) - 1000
    r = fresh_rows(rng, m)
    out = push_default(g, op, keys, r, np.ones(m, np.int64), 0)
    old = one_row_expected(r["a"], r["b"], r["c"])
    assert_one_row_step(out, keys, old, np.ones(m, np.int64), 0)
    # change every other key: retract its row, insert a different one
    sel = np.arange(0, m, 2)
    r2 = rows(r["a"][sel] + 1, r["b"][sel] - 1000, r["c"][sel] ^ 1)
    out = push_default(
        g, op, np.concatenate([keys[sel], keys[sel]]),
        np.concatenate([r[sel], r2]),
        np.concatenate([-np.ones(len(sel), np.int64),
                        np.ones(len(sel), np.int64)]), 1)
    assert_one_row_step(
        out, np.concatenate([keys[sel], keys[sel]]),
        np.concatenate([old[sel], one_row_expected(r2["a"], r2["b"],
                                                   r2["c"])]),
        np.concatenate([-np.ones(len(sel), np.int64),
                        np.ones(len(sel), np.int64)]), 1)
    g.collation_drop(op)


# 5 ------------------------------------------- table growth and compaction
def test_table_growth_and_compaction(g, monkeypatch):
    monkeypatch.setenv("MZ_GPU_COL_CAP", "64")
    rig = Rig(g)
    rng = np.random.default_rng(6)

    def batch(ids):
        return (np.asarray(ids).reshape(-1, 1),
                rows(rng.integers(-9, 9, len(ids)),
                     rng.integers(-99, 99, len(ids)),
                     rng.integers(-99, 99, len(ids))))

    k0, r0 = batch(np.arange(300))
    rig.step(k0, r0, np.ones(300, np.int64))          # 64 -> grows
    rig.step(k0[:200], r0[:200], -np.ones(200, np.int64))  # 200 dead rows
    k1, r1 = batch(np.arange(300, 500))
    rig.step(k1, r1, np.ones(200, np.int64))
    # 500 rows (200 dead) in a 512-row table: the next 100 new keys must
    # reclaim the dead rows; survivors keep their state across the rehash
    k2, r2 = batch(np.arange(500, 600))
    rig.step(k2, r2, np.ones(100, np.int64))
    k3, r3 = batch(np.arange(200, 600, 3))
    rig.step(k3, r3, np.ones(len(k3), np.int64))
    k4, r4 = batch(np.arange(0, 200))                   # rebirth after compaction
    rig.step(k4, r4, np.ones(200, np.int64))
    rig.drop()


# 6 ---------------------------- hierarchical-only and single-aggregate plans
def test_min_max_only(g):
    # no accumulable part; through the render surface
    plan = render.plan_reduce([MIN_B, MAX_C], abi.schema(1, ROW.itemsize),
                              buckets=BUCKETS)
    op = render.render_reduce(g, plan)
    assert isinstance(op, render.CollationOp)
    naive = Naive([MIN_B, MAX_C], 1)
    for t, (keys, vals, diffs) in enumerate(churn_stream(1, steps=4, n=600,
                                                         nkeys=40, seed=3)):
        dev = op.push(updates(keys, vals, diffs, t))
        assert dev.sorted
        got = out_rows(dev.to_host(), 1, 2 * SLOT)
        dev.release()
        assert got == naive.step(keys, vals, diffs, t), f"step {t}"
    op.drop()


def test_lone_max_equals_standalone_minmax(g):
    rig = Rig(g, aggs=[MAX_C])
    mm = g.minmax_create(abi.schema(1, 8), True, list(BUCKETS))
    for t, (keys, vals, diffs) in enumerate(churn_stream(1, steps=4, n=600,
                                                         nkeys=40, seed=3)):
        got = rig.step(keys, vals, diffs)
        proj = vals["c"].astype(np.int64)
        k, v, tm, d = g.minmax_push(mm, updates(keys, proj, diffs, t))
        relaid = sorted(
            ((int(k[i]),), bytes(8) + v[8 * i:8 * i + 8].tobytes() + bytes(8),
             int(tm[i]), int(d[i])) for i in range(len(tm)))
        assert got == relaid, f"step {t}"
    rig.drop()
    g.lib.mz_gpu_minmax_drop(g.ctx, mm)


def test_sum_f64_slot(g):
    # SUM_F64 beside a MIN: `a` carries an f64 here
    aggs = [COUNT, agg(abi.MZ_AGG_SUM_F64, 0, 8, is_float=1), MIN_B]
    rig = Rig(g, aggs=aggs)
    rng = np.random.default_rng(8)
    for _ in range(3):
        n = 300
        r = rows(np.zeros(n), rng.integers(-50, 50, n), np.zeros(n))
        x = rng.integers(-(1 << 20), 1 << 20, n) / 2.0  # multiples of 0.5
        r["a"] = x.view(np.int64)
        rig.step(rng.integers(0, 30, n).reshape(-1, 1), r,
                 np.ones(n, np.int64))
    rig.drop()


# 7 ------------------------------ cross-check against the existing operators
def maintain(state, out, kw, vb):
    keys, vals, _, diffs = out
    recs = [(tuple(int(x) for x in keys[i * kw:(i + 1) * kw]),
             vals[i * vb:(i + 1) * vb].tobytes(), int(diffs[i]))
            for i in range(len(diffs))]
    for k, v, d in recs:
        if d == -1:
            assert state.pop(k) == v
    for k, v, d in recs:
        if d == 1:
            assert k not in state
            state[k] = v
    assert all(d in (-1, 1) for _, _, d in recs)


@pytest.mark.parametrize("kw", [1, 2])
def test_cross_check_existing_operators(g, kw):
    sch = abi.schema(kw, ROW.itemsize)
    col = g.collation_create(abi.collation_spec(DEFAULT_AGGS, sch,
                                                buckets=BUCKETS))
    red = g.reduce_create(abi.reduce_spec([COUNT, SUM_A], sch))
    mn = g.minmax_create(abi.schema(kw, 8), False, list(BUCKETS))
    mx = g.minmax_create(abi.schema(kw, 8), True, list(BUCKETS))
    s_col, s_red, s_min, s_max = {}, {}, {}, {}
    for t, (keys, vals, diffs) in enumerate(churn_stream(kw)):
        maintain(s_col, g.collation_push(col, updates(keys, vals, diffs, t)),
                 kw, 4 * SLOT)
        maintain(s_red, g.reduce_push(red, updates(keys, vals, diffs, t)),
                 kw, 2 * SLOT)
        maintain(s_min, g.minmax_push(
            mn, updates(keys, vals["b"].copy(), diffs, t)), kw, 8)
        maintain(s_max, g.minmax_push(
            mx, updates(keys, vals["c"].astype(np.int64), diffs, t)), kw, 8)
        assert set(s_col) == set(s_red) == set(s_min) == set(s_max)
        for k, row in s_col.items():
            assert row[:2 * SLOT] == s_red[k], f"step {t} key {k}"
            assert row[2 * SLOT:3 * SLOT] == \
                bytes(8) + s_min[k] + bytes(8), f"step {t} key {k}"
            assert row[3 * SLOT:] == \
                bytes(8) + s_max[k] + bytes(8), f"step {t} key {k}"
    g.collation_drop(col)
    g.lib.mz_gpu_reduce_drop(g.ctx, red)
    for op in (mn, mx):
        g.lib.mz_gpu_minmax_drop(g.ctx, op)


# 8 ------------------------------------------------- loud errors, no faults
def test_multi_timestamp_push_raises(g):
    from materialize_amd._ffi import MzGpuError
    rig = Rig(g)
    u = updates(np.array([[1], [2]]), rows([1, 2], [1, 2], [1, 2]),
                np.array([1, 1]), 0, upper=2)
    with pytest.raises(MzGpuError, match="single-timestamp"):
        g.collation_push(rig.op, u)
    rig.step(np.array([[1]]), rows([1], [1], [1]), np.array([1]))
    rig.drop()


def test_partial_presence_raises_and_engine_survives(g):
    from materialize_amd._ffi import MzGpuError
    # total count 0, yet the bucket tree sees two non-zero vals: the key is
    # present in the MIN part only
    rig = Rig(g, aggs=[COUNT, MIN_B])
    u = updates(np.array([[7], [7], [8]]), rows([0, 0, 0], [3, 5, 1], [0] * 3),
                np.array([1, -1, 1]), 0)
    with pytest.raises(MzGpuError, match="missing a reduction type"):
        g.collation_push(rig.op, u)
    rig.drop()
    fresh = Rig(g, aggs=[COUNT, MIN_B])
    fresh.step(np.array([[7], [7], [8]]), rows([0, 0, 0], [3, 5, 1], [0] * 3),
               np.array([1, 1, 1]))
    fresh.step(np.array([[7]]), rows([0], [3], [0]), np.array([-1]))
    fresh.drop()


def test_reduce_create_rejects_min_max(g):
    from materialize_amd._ffi import MzGpuError
    for a in (MIN_B, MAX_C):
        with pytest.raises(MzGpuError, match="accumulable"):
            g.reduce_create(abi.reduce_spec([COUNT, a],
                                            abi.schema(1, ROW.itemsize)))


def raw_spec(**kw):
    sp = abi.collation_spec([COUNT, MIN_B], abi.schema(1, ROW.itemsize),
                            buckets=BUCKETS)
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def test_create_validates_in_c_too(g):
    """Specs built past the Python helper still fail loudly in the C
    layer."""
    from materialize_amd._ffi import MzGpuError
    bad = [raw_spec(n_aggs=0), raw_spec(n_aggs=5),
           raw_spec(in_=abi.schema(1, abi.MZ_GPU_VARLEN)),
           raw_spec(in_=abi.schema(1, 8)),            # MIN reads past
           raw_spec(out=abi.schema(1, 24)),
           raw_spec(n_levels=0), raw_spec(n_levels=5)]
    sp = raw_spec()
    sp.buckets[1] = 4                                  # last level != 1
    bad.append(sp)
    sp = raw_spec()
    sp.aggs[1].nullable = 1
    bad.append(sp)
    for sp in bad:
        with pytest.raises(MzGpuError, match="collation"):
            g.collation_create(sp)
