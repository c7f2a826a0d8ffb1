"""Open-addressing tables at their seams.

Every table in the engine probes with (h + 1) & (slots - 1). The keys
here are found on the host (valdomain.wrap_keys) so that their route hash
has its low 12 bits in {0xFFD, 0xFFE, 0xFFF}: in any table of <= 4096
slots they all start in the last three slots, so the collision cluster
runs off the end of the table and wraps to slot 0, and an absent key of
the same class starts its lookup inside that cluster and has to walk it,
around the end, to the first empty slot. Tables are filled in stages so
the wrapped cluster is rebuilt or rehashed at several sizes.

The second half pins the keyed-table capacity rule: whatever the
environment knobs ask for, a table's capacity is a power of two >= 16
(the probe mask needs it; a capacity of 48 or 100 would leave slots
unreachable and a full reachable subset makes the insert spin)."""
import numpy as np
import pytest

import test_collation_gpu as col
import test_distinct_aggs_gpu as dst
import valdomain as vd
from materialize_amd import _abi as abi

pytestmark = pytest.mark.gpu

N_ABSENT = 50


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def o():
    from pyoracle import OracleCtx
    ctx = OracleCtx()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def wrapped():
    """kw -> int64 [m, kw] keys of the wrapping hash class (kw = 2: word 0
    fixed at 5, the scan runs over word 1)."""
    return {1: vd.wrap_keys(1), 2: vd.wrap_keys(2, first_word=5)}


def test_wrap_keys_hash_class(g, wrapped):
    """The host hash the search runs on is the engine's, and the class is
    big enough for every test below."""
    from materialize_amd.dist import route_hash, shard_of
    for kw, keys in wrapped.items():
        assert len(keys) >= 2000
        sample = keys[:: len(keys) // 40]
        hs = route_hash(sample, kw)
        for k, h in zip(sample.tolist(), hs.tolist()):
            assert g.route_hash(k) == h
            assert h & 0xFFF >= 0xFFD
        np.testing.assert_array_equal(
            shard_of(sample, kw, 7), (hs % np.uint64(7)).astype(np.int64))
    for slots in (16, 64, 512, 4096):  # all start in the last three slots
        home = route_hash(wrapped[1][:300], 1) & np.uint64(slots - 1)
        assert home.min() >= slots - 3


# ------------------------------------------------------- the batch hash

def arr_batch(keys, t, salt):
    """One update per key at time t; the payload names the key's row."""
    n = len(keys)
    v = (np.arange(n, dtype=np.int64) * 7 + salt)
    return (keys, v.view(np.uint8).reshape(n, 8).copy(),
            np.full(n, t, np.uint64), np.ones(n, np.int64))


@pytest.mark.parametrize("layout", ["one", "several", "maintained"])
@pytest.mark.parametrize("nkeys", [24, 200])
@pytest.mark.parametrize("kw", [1, 2])
def test_batch_hash_wraps(g, o, wrapped, kw, nkeys, layout):
    """halfjoin, peek and join_push over batches whose hash tables hold
    one wrapped cluster: one batch; three batches of different sizes;
    and their merge, which rebuilds the table at another size."""
    present = wrapped[kw][:nkeys]
    absent = wrapped[kw][nkeys:nkeys + N_ABSENT]
    sch = abi.schema(kw, 8)
    ga, oa = g.arr_create(sch), o.arr_create(sch)
    if layout == "one":
        batches = [arr_batch(present, 0, 1)]
    else:  # 1/8, 3/8 and all of the keys: tables of three sizes
        batches = [arr_batch(present[:nkeys // 8], 0, 1),
                   arr_batch(present[nkeys // 8:nkeys // 2], 1, 2),
                   arr_batch(present, 2, 3)]
    for t, b in enumerate(batches):
        u = vd.updates(abi, b, t, t + 1)
        g.arr_insert(ga, u)
        o.arr_insert(oa, u)
    if layout == "maintained":
        g.arr_maintain(ga)
        o.arr_maintain(oa)
        assert g.arr_stats(ga)[0] == 1
    T = 5
    pk = np.concatenate([present, absent])
    pk = pk[np.random.default_rng(nkeys).permutation(len(pk))]
    n = len(pk)
    stream = (pk, np.zeros((n, 0), np.uint8), np.full(n, T, np.uint64),
              np.ones(n, np.int64))
    su = vd.updates(abi, stream, T, T + 1)
    cl = vd.probe_closure(abi, kw)
    want = vd.naive_halfjoin(stream, batches, kw, True)
    assert {r[0] for r in want} == {tuple(k) for k in present.tolist()}
    got = g.halfjoin(ga, su, 0, True, cl)
    assert vd.to_rows(*got, kw, 8) == want, "halfjoin vs naive"
    vd.assert_cols_equal(got, o.halfjoin(oa, su, 0, True, cl), "halfjoin")
    got = g.peek(ga, pk, T, kw)
    assert vd.to_rows(*got, kw, 8) == vd.naive_as_of(batches, T, kw, 8), \
        "peek vs naive"
    vd.assert_cols_equal(got, o.peek(oa, pk, T, kw), "peek")
    # join_push: the delta enters side 1 and probes the wrapped batches
    jcl = abi.closure([], [abi.field(abi.MZ_SRC_KEY, 0, 8 * kw)],
                      [abi.field(abi.MZ_SRC_VAL_STREAM, 0, 8),
                       abi.field(abi.MZ_SRC_VAL_LOOKUP, 0, 8)],
                      abi.schema(kw, 16))
    delta = arr_batch(pk, T, 1000)
    res = []
    for ctx, arr2 in ((g, ga), (o, oa)):
        arr1 = ctx.arr_create(sch)
        op = ctx.join_create(arr1, arr2, jcl)
        k, v, t, d = ctx.consolidate(sch, vd.updates(abi, delta, T, T + 1))
        sealed = abi.make_updates(k, v, t, d, T, T + 1)
        ctx.arr_push(arr1, sealed)
        res.append(ctx.join_push(op, 1, sealed))
    vd.assert_cols_equal(res[0], res[1], "join_push")
    jrows = vd.to_rows(*res[0], kw, 16)
    assert {r[0] for r in jrows} == {tuple(k) for k in present.tolist()}
    assert len(jrows) == sum(len(b[2]) for b in batches)


# ----------------------------------------------------- the keyed tables

def staged(keys, sizes):
    """Consecutive slices of `keys` of the given sizes."""
    out, at = [], 0
    for s in sizes:
        out.append(keys[at:at + s])
        at += s
    return out


def i64_vals(x):
    x = np.ascontiguousarray(x, np.int64)
    return x.view(np.uint8).reshape(len(x), 8).copy()


def reduce_parity(g, o, kw, pushes, what):
    """SUM_I64 + COUNT over the pushes (keys, i64 vals, diffs), one
    timestamp each, GPU against oracle; returns the corrections."""
    spec = vd.sum_count_spec(abi, kw)
    gop, oop = g.reduce_create(spec), o.reduce_create(spec)
    outs = []
    for t, (keys, v, d) in enumerate(pushes):
        u = abi.make_updates(keys.ravel(), i64_vals(v).ravel(),
                             np.full(len(d), t, np.uint64),
                             np.asarray(d, np.int64), t, t + 1)
        got = g.reduce_push(gop, u)
        vd.assert_cols_equal(got, o.reduce_push(oop, u), f"{what} push {t}")
        outs.append(vd.to_rows(*got, kw, 48))
    g.reduce_drop(gop)
    return outs


def count_of(row):
    """(retracted?, COUNT) of a correction row of sum_count_spec."""
    return row[3], row[1][4]


@pytest.mark.parametrize("kw", [1, 2])
def test_reduce_table_wraps_and_rehashes(g, o, wrapped, kw, monkeypatch):
    """32 rows -> 64 slots: 24 wrapping keys fit without growth; two
    growths (kt_compact_grow / k_rehash_rows) then rehash the wrapped
    cluster at 256 and 512 slots. Afterwards every key must be found
    with its payload (its retraction names the old count) and 50 absent
    keys of the class must miss (they open fresh groups)."""
    monkeypatch.setenv("MZ_GPU_RED_CAP", "32")
    keys = wrapped[kw]
    s1, s2, s3, absent = staged(keys, [24, 60, 120, N_ABSENT])
    present = np.concatenate([s1, s2, s3])
    n = len(present)
    pushes = [(s, np.arange(len(s)) + 10, np.ones(len(s), np.int64))
              for s in (s1, s2, s3)]
    pushes.append((present, np.full(n, 3), np.full(n, 2, np.int64)))
    pushes.append((absent, np.full(N_ABSENT, 4),
                   np.ones(N_ABSENT, np.int64)))
    outs = reduce_parity(g, o, kw, pushes, "reduce wrap")
    # found: each present key retracts COUNT 1 and asserts COUNT 3
    assert len(outs[3]) == 2 * n
    assert sorted(count_of(r) for r in outs[3]) == \
        [(-1, 1)] * n + [(1, 3)] * n
    # missed: the absent keys have no old row to retract
    assert [count_of(r) for r in outs[4]] == [(1, 1)] * N_ABSENT


def threshold_parity(g, o, sch, pushes, what):
    gop, oop = g.threshold_create(sch), o.threshold_create(sch)
    outs = []
    for t, (keys, v, d) in enumerate(pushes):
        u = abi.make_updates(keys.ravel(), i64_vals(v).ravel(),
                             np.full(len(d), t, np.uint64),
                             np.asarray(d, np.int64), t, t + 1)
        got = g.threshold_push(gop, u)
        vd.assert_cols_equal(got, o.threshold_push(oop, u),
                             f"{what} push {t}")
        outs.append(vd.to_rows(*got, sch.key_words, 8))
    return outs


def test_threshold_table_wraps_and_rehashes(g, o, wrapped, monkeypatch):
    """The threshold table is keyed by (key word, val word): the wrapping
    rows are key 5 with the class's second words as vals. 64 rows -> 128
    slots, then two growths."""
    monkeypatch.setenv("MZ_GPU_THR_CAP", "64")
    rows = wrapped[2]
    s1, s2, s3, absent = staged(rows, [40, 100, 60, N_ABSENT])
    present = np.concatenate([s1, s2, s3])
    n = len(present)
    one = lambda r, d: (r[:, :1], r[:, 1], np.full(len(r), d, np.int64))
    pushes = [one(s1, 2), one(s2, 2), one(s3, 2),
              one(present, -1),   # found: count 2 -> 1, emits -1 each
              one(absent, -1),    # missed: count -1, nothing to emit
              one(absent, 3)]     # -1 -> 2, emits +2 each
    outs = threshold_parity(g, o, abi.schema(1, 8), pushes, "threshold wrap")
    assert [r[3] for r in outs[3]] == [-1] * n
    assert outs[4] == []
    assert [r[3] for r in outs[5]] == [2] * N_ABSENT


def test_distinct_pair_table_wraps_and_rehashes(g, wrapped, monkeypatch):
    """COUNT(DISTINCT a) keeps a (key, datum) -> count table: group key 5
    with the class's second words as datums. 32 rows -> 64 slots, two
    growths, then retractions and returns of pairs inside the cluster.
    The reference is test_distinct_aggs_gpu's naive model (the oracle's
    reduce has no distinct aggregates)."""
    monkeypatch.setenv("MZ_GPU_RED_CAP", "32")
    rig = dst.Rig(g, [dst.COUNT_D_A, dst.COUNT])
    datums = wrapped[2][:, 1]
    s1, s2, s3, absent = staged(datums, [24, 60, 120, N_ABSENT])
    present = np.concatenate([s1, s2, s3])
    steps = [(s1, 1), (s2, 1), (s3, 1),
             (present, 1),         # every pair found: no new distinct datum
             (present[::2], -2),   # half the pairs leave
             (absent, 1),          # missed: 50 new distinct datums
             (present[::2], 1)]    # the pairs that left come back
    counts = []
    for d, diff in steps:
        keys = np.full((len(d), 1), 5, np.int64)
        diffs = np.full(len(d), diff, np.int64)
        rig.step(keys, dst.rows(d), diffs)  # asserts GPU == model
        (_, row), = rig.naive.rows.items()
        counts.append(dst.count_of(row, 0))
    assert counts == [24, 84, 204, 204, 102, 152, 254]
    rig.drop()


def test_collation_table_wraps_and_rehashes(g, wrapped, monkeypatch):
    """The collation's stitch table, 64 rows -> 128 slots, two growths,
    a retraction wave that leaves dead rows inside the wrapped cluster,
    and a return. The reference is test_collation_gpu's naive model (the
    oracle has no collated operator)."""
    monkeypatch.setenv("MZ_GPU_COL_CAP", "64")
    rig = col.Rig(g)
    rng = np.random.default_rng(5)
    s1, s2, s3, absent = staged(wrapped[1], [40, 100, 100, N_ABSENT])
    present = np.concatenate([s1, s2, s3])
    memo = {}

    def step(keys, diff):
        r = col.rows(*(rng.integers(-99, 99, len(keys)) for _ in range(3)))
        if diff > 0:
            memo.update(zip(keys[:, 0].tolist(), r))
        else:  # retract exactly the row that went in
            r = np.array([memo[k] for k in keys[:, 0].tolist()], col.ROW)
        return rig.step(keys, r, np.full(len(keys), diff, np.int64))

    for s in (s1, s2, s3):
        assert len(step(s, 1)) == len(s)
    assert len(step(present[::3], -1)) == len(present[::3])
    assert len(step(absent, 1)) == N_ABSENT      # missed: new groups only
    assert len(step(present[::3], 1)) == len(present[::3])
    assert len(step(present[1::3], -1)) == len(present[1::3])
    rig.drop()


# --------------------------------------------- capacity knobs are rounded

def churn_pushes(rng, nkeys, steps, n):
    keys = np.arange(nkeys, dtype=np.int64) * 3 - nkeys
    out = []
    for _ in range(steps):
        out.append((keys[rng.integers(0, nkeys, n)].reshape(n, 1),
                    rng.integers(-50, 50, n),
                    rng.choice(np.array([-1, 1, 1, 2], np.int64), n)))
    return out


@pytest.mark.parametrize("cap", ["48", "0"])
def test_reduce_capacity_is_rounded(g, o, cap, monkeypatch):
    """MZ_GPU_RED_CAP that is no power of two (or zero): about 300
    distinct keys, at least two growths on top of the rounded capacity."""
    monkeypatch.setenv("MZ_GPU_RED_CAP", cap)
    rng = np.random.default_rng(48)
    pushes = churn_pushes(rng, 300, 5, 120)
    outs = reduce_parity(g, o, 1, pushes, f"RED_CAP={cap}")
    assert len({r[0] for out in outs for r in out}) > 200


@pytest.mark.parametrize("cap", ["100", "0"])
def test_threshold_capacity_is_rounded(g, o, cap, monkeypatch):
    monkeypatch.setenv("MZ_GPU_THR_CAP", cap)
    rng = np.random.default_rng(100)
    pushes = [(k, v % 2, d) for k, v, d in churn_pushes(rng, 300, 5, 150)]
    outs = threshold_parity(g, o, abi.schema(1, 8), pushes,
                            f"THR_CAP={cap}")
    assert len({r[:2] for out in outs for r in out}) > 200
