"""DISTINCT aggregates on the GPU: COUNT(DISTINCT x) / SUM(DISTINCT x) in the
accumulable reduce and behind the collation, against a naive full recompute.

The oracle has no DISTINCT, so the reference lives here (the style of
tests/test_collation_gpu.py): the model is key -> multiset of val rows;
after each timestamp the finalized row of every live key is computed from
scratch and the expected corrections are the difference from the previous
rows. Everything compares bit-exact as sorted (key, val bytes, time, diff).

Input rows are 24 bytes. ROW: a = i64 @0, b = i64 @8, c = i32 @16, pad.
NROW (nullable datums, indicator byte at off + width): x = i64 @0, xn = u8
@8, y = i32 @12, yn = u8 @16, pad.
"""
import struct

import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

pytestmark = pytest.mark.gpu

ROW = np.dtype([("a", "<i8"), ("b", "<i8"), ("c", "<i4"), ("pad", "<i4")])
NROW = np.dtype([("x", "<i8"), ("xn", "u1"), ("p0", "u1", 3), ("y", "<i4"),
                 ("yn", "u1"), ("p1", "u1", 7)])
assert ROW.itemsize == NROW.itemsize == 24
SLOT = abi.AGG_SLOT_BYTES
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def agg(func, off=0, width=8, nullable=0, distinct=0, is_float=0):
    return abi.Aggregate(func=func, off=off, width=width, is_float=is_float,
                         nullable=nullable, distinct=distinct)


COUNT = agg(abi.MZ_AGG_COUNT)
SUM_A = agg(abi.MZ_AGG_SUM_I64, 0)
COUNT_D_A = agg(abi.MZ_AGG_COUNT, 0, distinct=1)
SUM_D_A = agg(abi.MZ_AGG_SUM_I64, 0, distinct=1)
COUNT_D_C = agg(abi.MZ_AGG_COUNT, 16, 4, distinct=1)
SUM_D_C = agg(abi.MZ_AGG_SUM_I64, 16, 4, distinct=1)
MIN_B = agg(abi.AGG_MIN_I64, 8)
BUCKETS = (16, 1)


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


def rows(a, b=None, c=None):
    a = np.asarray(a, np.int64)
    r = np.zeros(len(a), ROW)
    r["a"] = a
    r["b"] = 0 if b is None else b
    r["c"] = 0 if c is None else c
    return r


def nrows(x, y):
    """None = NULL (the datum bytes of a NULL are arbitrary: 77 here)."""
    r = np.zeros(len(x), NROW)
    r["x"] = [77 if v is None else v for v in x]
    r["xn"] = [v is None for v in x]
    r["y"] = [77 if v is None else v for v in y]
    r["yn"] = [v is None for v in y]
    return r


def updates(keys, vals, diffs, times, lower, upper):
    keys = np.ascontiguousarray(keys, np.int64)
    return abi.make_updates(keys.ravel(), vals.view(np.uint8).ravel(),
                            np.asarray(times, np.uint64),
                            np.asarray(diffs, np.int64), lower, upper)


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


def is_null(v, a):
    return bool(a.nullable) and v[a.off + a.width] != 0


def slot(a, counter):
    """Finalized 24-byte slot of aggregate `a` over {val bytes: count}."""
    s = bytearray(SLOT)
    if abi.is_hierarchical(a):
        vals = [datum(v, a) for v in counter]
        m = max(vals) if a.func == abi.AGG_MAX_I64 else min(vals)
        s[8:16] = struct.pack("<q", m)
        return bytes(s)
    total = sum(counter.values())
    live = [(v, c) for v, c in counter.items() if not is_null(v, a)]
    if a.distinct:
        net = {}
        for v, c in live:
            net[datum(v, a)] = net.get(datum(v, a), 0) + c
        present = [d for d, c in net.items() if c != 0]
        nn, acc = len(present), sum(present)
    else:
        nn = sum(c for _, c in live)
        acc = 0
        if a.func == abi.MZ_AGG_SUM_I64:
            acc = sum(datum(v, a) * c for v, c in live)
    if a.func == abi.MZ_AGG_COUNT:
        s[8:16] = struct.pack("<q", nn)
    elif total > 0 and nn == 0 and acc % (1 << 128) == 0:
        s[0] = 1                      # SUM over no non-null datum: NULL
    else:
        s[8:24] = (acc % (1 << 128)).to_bytes(16, "little")
    return bytes(s)


NULL_SLOT = bytes([1]) + bytes(SLOT - 1)


def count_of(row, i):
    return struct.unpack_from("<q", row, i * SLOT + 8)[0]


def sum_of(row, i):
    assert row[i * SLOT] == 0
    return int.from_bytes(row[i * SLOT + 8:i * SLOT + 24], "little",
                          signed=True)


class Naive:
    def __init__(self, aggs, kw):
        self.aggs, self.kw = list(aggs), kw
        self.model = {}   # key tuple -> {val bytes: count}
        self.rows = {}    # key tuple -> finalized row after the last time

    def step(self, keys, vals, diffs, times):
        """Apply the updates in time order; corrections per timestamp."""
        keys = np.asarray(keys, np.int64).reshape(-1, self.kw)
        raw = vals.view(np.uint8).reshape(len(diffs), -1)
        times = np.asarray(times)
        exp = []
        for t in sorted(set(int(x) for x in times)):
            for k, v, d, tt in zip(keys, raw, diffs, times):
                if int(tt) != t:
                    continue
                k, v = tuple(int(x) for x in k), v.tobytes()
                cnt = self.model.setdefault(k, {})
                cnt[v] = cnt.get(v, 0) + int(d)
                assert cnt[v] >= 0, "the streams keep multiplicities >= 0"
                if cnt[v] == 0:
                    del cnt[v]
                if not cnt:
                    del self.model[k]
            new = {k: b"".join(slot(a, cnt) for a in self.aggs)
                   for k, cnt in self.model.items()}
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
    """An operator (plain reduce, or the collation when MIN/MAX are among
    the aggregates) and its naive model, stepped together."""

    def __init__(self, g, aggs, kw=1):
        self.g, self.kw = g, kw
        self.aggs = list(aggs)
        self.vb = SLOT * len(self.aggs)
        plan = render.plan_reduce(self.aggs, abi.schema(kw, 24),
                                  **({"buckets": BUCKETS} if any(
                                      abi.is_hierarchical(a)
                                      for a in self.aggs) else {}))
        self.op = render.render_reduce(g, plan)
        self.naive = Naive(self.aggs, kw)
        self.t = 0

    def step(self, keys, vals, diffs, times=None):
        """One push. `times` (offsets from the push's lower bound) makes it
        a multi-timestamp push."""
        n = len(diffs)
        rel = np.zeros(n, np.int64) if times is None else np.asarray(times)
        lower = self.t
        upper = lower + int(rel.max(initial=0)) + 1
        self.t = upper
        dev = self.op.push(updates(keys, vals, diffs, lower + rel, lower,
                                   upper))
        out = dev.to_host()
        dev.release()
        got = out_rows(out, self.kw, self.vb)
        want = self.naive.step(keys, vals, diffs, lower + rel)
        assert got == want, f"push at {lower}"
        if upper == lower + 1:
            assert_canonical_keys(out, self.kw)
        return got

    def drop(self):
        self.op.drop()


def key_words(k, kw):
    """kw = 2 spreads the ids over both words, negatives included."""
    k = np.asarray(k, np.int64)
    if kw == 1:
        return (k - 50).reshape(-1, 1)
    return np.stack([k % 7 - 3, k // 7 - 5], axis=1)


# 1 ------------------------------------------------------------ transitions
def test_pair_transitions(g):
    rig = Rig(g, [COUNT_D_A, SUM_D_A, COUNT, SUM_A])
    K = np.array([[3]])

    def decoded(got):
        return sorted((d, count_of(v, 0), sum_of(v, 1), count_of(v, 2),
                       sum_of(v, 3)) for _, v, _, d in got)

    # pair (3, 5): 0 -> 1
    assert decoded(rig.step(K, rows([5], [1]), [1])) == [(1, 1, 5, 1, 5)]
    # 1 -> 2 (another row with the same a): distinct slots stay, plain move
    assert decoded(rig.step(K, rows([5], [2]), [1])) == [
        (-1, 1, 5, 1, 5), (1, 1, 5, 2, 10)]
    # a second pair (3, 7): 0 -> 1
    assert decoded(rig.step(K, rows([7], [1]), [1])) == [
        (-1, 1, 5, 2, 10), (1, 2, 12, 3, 17)]
    # pair (3, 5): 2 -> 1
    assert decoded(rig.step(K, rows([5], [2]), [-1])) == [
        (-1, 2, 12, 3, 17), (1, 2, 12, 2, 12)]
    # pair (3, 7): 1 -> 0
    assert decoded(rig.step(K, rows([7], [1]), [-1])) == [
        (-1, 2, 12, 2, 12), (1, 1, 5, 1, 5)]
    # +1 and -1 of one pair in one push — a new pair (3, 9), and the
    # resident one (3, 5) through two different rows: nothing changes
    assert rig.step(np.array([[3], [3]]), rows([9, 9], [4, 4]), [1, -1]) == []
    assert decoded(rig.step(np.array([[3], [3]]), rows([5, 5], [1, 6]),
                            [-1, 1])) == []
    # the key vanishes ...
    assert decoded(rig.step(K, rows([5], [6]), [-1])) == [(-1, 1, 5, 1, 5)]
    # ... and comes back, with a pair the table has seen and a fresh one
    assert decoded(rig.step(np.array([[3], [3]]), rows([5, -2], [1, 1]),
                            [1, 1])) == [(1, 2, 3, 2, 3)]
    rig.drop()


# 2 ----------------------------------------------------------- random churn
UNIVERSE_A = np.array([-(1 << 40), -7, -1, 0, 1, 2, 1 << 33, 1 << 50])
UNIVERSE_C = np.array([-(1 << 31), -1000, -2, -1, 0, 1, 3, (1 << 31) - 1])


def churn_stream(kw, seed=21, steps=12, n=500, nkeys=300):
    """Inserts with multiplicity 1..3 and retractions of part of a present
    row's multiplicity; datums from 8-value universes, so most pairs are
    held by several rows. Per step (keys[n,kw], rows[n], diffs[n])."""
    rng = np.random.default_rng(seed)
    present, out = {}, []       # (key id, a, b, c) -> multiplicity
    for _ in range(steps):
        ks, rs, ds = [], [], []
        for _ in range(n):
            if present and rng.random() < 0.45:
                rec = list(present)[int(rng.integers(0, len(present)))]
                d = -int(rng.integers(1, present[rec] + 1))
            else:
                rec = (int(rng.integers(0, nkeys)),
                       int(UNIVERSE_A[rng.integers(0, 8)]),
                       int(rng.integers(0, 3)),
                       int(UNIVERSE_C[rng.integers(0, 8)]))
                d = int(rng.integers(1, 4))
            present[rec] = present.get(rec, 0) + d
            if present[rec] == 0:
                del present[rec]
            ks.append(rec[0])
            rs.append(rec[1:])
            ds.append(d)
        a, b, c = (np.array(x) for x in zip(*rs))
        out.append((key_words(ks, kw), rows(a, b, c), np.array(ds, np.int64)))
    return out


@pytest.mark.parametrize("kw", [1, 2])
def test_random_churn(g, kw):
    rig = Rig(g, [COUNT_D_A, SUM_D_C, COUNT, SUM_D_A], kw=kw)
    changed = 0
    for keys, vals, diffs in churn_stream(kw):
        changed += len(rig.step(keys, vals, diffs))
    assert changed > 300  # the stream did exercise the operator
    rig.drop()


# 3 ------------------------------------------------------------------ NULLs
def test_null_datums(g):
    cd_x = agg(abi.MZ_AGG_COUNT, 0, 8, nullable=1, distinct=1)
    sd_x = agg(abi.MZ_AGG_SUM_I64, 0, 8, nullable=1, distinct=1)
    sd_y = agg(abi.MZ_AGG_SUM_I64, 12, 4, nullable=1, distinct=1)
    rig = Rig(g, [cd_x, sd_x, COUNT, sd_y])
    # keys 0 and 9 — the first and the last of the slice — hold only NULLs
    keys = np.array([0, 0, 1, 1, 1, 4, 4, 9]).reshape(-1, 1)
    x = [None, None, 5, 5, None, -3, 8, None]
    y = [None, None, -1, -1, 2, None, None, None]
    got = rig.step(keys, nrows(x, y), [1, 2, 1, 1, 1, 1, 1, 1])
    by_key = {k[0]: v for k, v, _, _ in got}
    for k, n_rows in ((0, 3), (9, 1)):
        v = by_key[k]
        assert count_of(v, 0) == 0 and count_of(v, 2) == n_rows
        assert v[SLOT:2 * SLOT] == NULL_SLOT and v[3 * SLOT:] == NULL_SLOT
    assert (count_of(by_key[1], 0), sum_of(by_key[1], 1),
            sum_of(by_key[1], 3)) == (1, 5, 1)
    assert by_key[4][3 * SLOT:] == NULL_SLOT and sum_of(by_key[4], 1) == 5
    # all-NULL -> has a value (0: a datum equal to the neutral one)
    got = rig.step(np.array([[0], [9]]), nrows([0, 6], [None, 0]), [1, 1])
    new = {k[0]: v for k, v, _, d in got if d == 1}
    assert (count_of(new[0], 0), sum_of(new[0], 1)) == (1, 0)
    assert new[0][3 * SLOT:] == NULL_SLOT
    assert (count_of(new[9], 0), sum_of(new[9], 1), sum_of(new[9], 3)) == \
        (1, 6, 0)
    # ... and back to all-NULL
    got = rig.step(np.array([[0], [9]]), nrows([0, 6], [None, 0]), [-1, -1])
    new = {k[0]: v for k, v, _, d in got if d == 1}
    for k in (0, 9):
        assert count_of(new[k], 0) == 0
        assert new[k][SLOT:2 * SLOT] == NULL_SLOT
        assert new[k][3 * SLOT:] == NULL_SLOT
    # a NULL and a value of one key, retracted and re-added in one push
    rig.step(np.array([[1], [1], [1]]), nrows([None, 5, 5], [2, -1, 7]),
             [-1, -1, 1])
    rig.drop()


# 4 ---------------------------------------------------- multi-timestamp push
def test_multi_timestamp_push(g):
    aggs = [COUNT_D_A, SUM_D_A, COUNT]
    multi, single = Rig(g, aggs), Rig(g, aggs)
    both = (multi, single)
    for r in both:
        r.step(np.array([[1], [2]]), rows([10, 20]), [1, 1])
    # key 1: pair (1, 11) inserted at t and retracted at t + 1;
    # key 2: pair (2, 21) inserted at both times; key 5 appears at t + 1
    keys = np.array([1, 1, 2, 2, 5]).reshape(-1, 1)
    vals = rows([11, 11, 21, 21, 50])
    diffs = np.array([1, -1, 1, 1, 1])
    rel = np.array([0, 1, 0, 1, 1])
    got = multi.step(keys, vals, diffs, times=rel)
    t = single.t
    one_by_one = []
    for dt in (0, 1):
        sel = rel == dt
        one_by_one += single.step(keys[sel], vals[sel], diffs[sel])
    assert got == sorted(one_by_one)
    at = lambda tt: sorted((k[0], d, count_of(v, 0), sum_of(v, 1),
                            count_of(v, 2))
                           for k, v, tm, d in got if tm == tt)
    assert at(t) == [(1, -1, 1, 10, 1), (1, 1, 2, 21, 2),
                     (2, -1, 1, 20, 1), (2, 1, 2, 41, 2)]
    assert at(t + 1) == [(1, -1, 2, 21, 2), (1, 1, 1, 10, 1),
                         (2, -1, 2, 41, 2), (2, 1, 2, 41, 3),
                         (5, 1, 1, 50, 1)]
    assert {tm for _, _, tm, _ in got} == {t, t + 1}
    for r in both:
        r.drop()


# 5 --------------------------------------------------------------- extremes
def test_extremes(g):
    rig = Rig(g, [SUM_D_A, COUNT_D_A, SUM_D_C, COUNT_D_C])
    a = [I64_MAX, I64_MAX, I64_MAX - 1, I64_MIN, I64_MIN]
    got = rig.step(np.zeros((5, 1), np.int64), rows(a, range(5), [-1] * 5),
                   [1, 2, 1, 3, 1])
    (_, v, _, d), = got
    # each datum once: MAX + (MAX - 1) + MIN = 2^63 - 3, past i64
    assert d == 1 and sum_of(v, 0) == (1 << 63) - 3 and count_of(v, 1) == 3
    # the i32 -1 enters the sum as -1, not as 0xFFFFFFFF
    assert sum_of(v, 2) == -1 and count_of(v, 3) == 1
    assert v[2 * SLOT + 8:3 * SLOT] == b"\xff" * 16
    # ... and an i64 datum 0xFFFFFFFF is a different value from -1
    got = rig.step(np.ones((2, 1), np.int64),
                   rows([-1, 0xFFFFFFFF], [0, 0], [-1, 0]), [1, 1])
    (_, v, _, _), = got
    assert count_of(v, 1) == 2 and sum_of(v, 0) == 0xFFFFFFFE
    assert count_of(v, 3) == 2 and sum_of(v, 2) == -1
    rig.drop()


# 6 ----------------------------------------------------------------- growth
def test_pair_table_growth(g, monkeypatch):
    monkeypatch.setenv("MZ_GPU_RED_CAP", "32")
    rig = Rig(g, [COUNT_D_A, SUM_D_A, COUNT])
    ids = np.arange(200)
    keys = (ids % 40).reshape(-1, 1)
    rig.step(keys, rows(ids * 3), np.ones(200, np.int64))    # 32 -> grows
    half = ids[::2]
    rig.step(keys[half], rows(half * 3), -np.ones(100, np.int64))
    rig.step(keys, rows(1000 + ids), np.ones(200, np.int64))
    # 400 rows, 100 of them dead, in tables of 512: the next 200 new pairs
    # must reclaim the dead rows; survivors keep their counts
    rig.step(keys, rows(2000 + ids), np.ones(200, np.int64))
    # the reclaimed half comes back
    rig.step(keys[half], rows(half * 3), np.ones(100, np.int64))
    assert len(rig.naive.rows) == 40
    assert all(count_of(v, 0) == 15 for v in rig.naive.rows.values())
    rig.drop()


# 7 -------------------------------------------------------------- collation
def test_distinct_behind_the_collation(g):
    rig = Rig(g, [COUNT_D_A, MIN_B, SUM_A])
    assert isinstance(rig.op, render.CollationOp)
    for keys, vals, diffs in churn_stream(1, seed=5, steps=5, n=300,
                                          nkeys=40):
        rig.step(keys, vals, diffs)
    rig.drop()


# 8 -------------------------------------------------------- rejected shapes
def test_c_layer_rejects_unsupported_distinct(g):
    """Specs filled by hand, past _abi's checks, fail loudly in C."""
    from materialize_amd._ffi import MzGpuError
    sch = abi.schema(1, 24)

    def forced(sp, **fields):
        sp.aggs[0].distinct = 1
        for k, v in fields.items():
            setattr(sp.aggs[0], k, v)
        return sp

    plain_f64 = agg(abi.MZ_AGG_SUM_F64, 0, 8, is_float=1)
    with pytest.raises(MzGpuError, match="DISTINCT over a float datum"):
        g.reduce_create(forced(abi.reduce_spec([plain_f64], sch)))
    with pytest.raises(MzGpuError, match="DISTINCT over a float datum"):
        g.reduce_create(forced(abi.reduce_spec([SUM_A], sch), is_float=1))
    with pytest.raises(MzGpuError, match="DISTINCT datum width"):
        g.reduce_create(forced(abi.reduce_spec([COUNT], sch), width=2))
    with pytest.raises(MzGpuError, match="DISTINCT datum reads past"):
        g.reduce_create(forced(abi.reduce_spec([COUNT], sch), off=20))
    with pytest.raises(MzGpuError,
                       match="collation: DISTINCT over a float datum"):
        g.collation_create(forced(abi.collation_spec([plain_f64, MIN_B], sch,
                                                     buckets=BUCKETS)))
    with pytest.raises(MzGpuError, match="collation: DISTINCT datum reads"):
        g.collation_create(forced(abi.collation_spec([COUNT, MIN_B], sch,
                                                     buckets=BUCKETS),
                                  off=17))
    # the context is intact: MIN/MAX take the flag and ignore it
    rig = Rig(g, [agg(abi.AGG_MIN_I64, 8, distinct=1), COUNT_D_A])
    rig.step(np.array([[1], [1]]), rows([4, 4], [9, 2]), [1, 1])
    rig.drop()
