"""Single-time reduce pushes emit their corrections in canonical order with
no sort behind them: group g of the push writes its 0, 1 or 2 rows to
staging slots 2g and 2g + 1, the row whose val comes first in the canonical
val order first, and one scan + one compaction make the result.

Two operators over i64 vals: SUM_I64 + COUNT, and SUM_I64 + COUNT(DISTINCT).
Every key here holds distinct datums of multiplicity one, so COUNT(DISTINCT)
equals COUNT and ONE reference serves both: the CPU oracle's reduce over
the same pushes, compared byte for byte and in order. The second check is
the property that makes dropping the re-sort legal: consolidating the
output returns it unchanged.

Key classes of a push (by group index mod 6) against a state in which every
existing key holds one row a = 10:
  0 created     (5, +1)                 only a +1 row
  1 deleted     (10, -1)                only a -1 row
  2 sum up      (10, -1), (25, +1)      new val after old
  3 sum down    (10, -1), (4, +1)       new val before old
  4 below zero  (10, -1), (-15, +1)     the sum's low word flips to
                                        0xFF..F1: new val after old although
                                        the sum fell
  5 unchanged   (7, +1), (7, -1)        emits nothing"""
import numpy as np
import pytest

import valdomain as vd
from materialize_amd import _abi as abi

pytestmark = pytest.mark.gpu

GRID_CAP_GROUPS = 2048 * 256
CLASS_ROWS = {0: [(5, 1)], 1: [(10, -1)], 2: [(10, -1), (25, 1)],
              3: [(10, -1), (4, 1)], 4: [(10, -1), (-15, 1)],
              5: [(7, 1), (7, -1)]}
ROWS_OUT = {0: 1, 1: 1, 2: 2, 3: 2, 4: 2, 5: 0}
OPS = ["plain", "distinct"]


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


def agg(func, distinct=0):
    return abi.Aggregate(func=func, off=0, width=8, is_float=0, nullable=0,
                         distinct=distinct)


def spec_of(op):
    if op == "plain":
        return vd.sum_count_spec(abi, 1)
    return abi.reduce_spec([agg(abi.MZ_AGG_SUM_I64),
                            agg(abi.MZ_AGG_COUNT, distinct=1)],
                           abi.schema(1, 8))


def upd(rows, lower, upper):
    """rows: (keys, a, times, diffs) arrays -> host Updates."""
    k, a, t, d = (np.asarray(x) for x in rows)
    return abi.make_updates(k.astype(np.int64),
                            a.astype(np.int64).view(np.uint8),
                            t.astype(np.uint64), d.astype(np.int64),
                            lower, upper)


def cat(*rows):
    return tuple(np.concatenate([np.asarray(r[i]) for r in rows])
                 for i in range(4))


EMPTY = (np.zeros(0, np.int64),) * 4


def state_and_push(classes, rng):
    """For group classes (one per key, keys ascending from a negative id):
    the rows that build the state at time 0 and the shuffled rows of the
    push at time 1."""
    classes = np.asarray(classes)
    keys = np.arange(len(classes), dtype=np.int64) - len(classes) // 2
    old = keys[classes != 0]
    state = (old, np.full(len(old), 10), np.zeros(len(old)),
             np.ones(len(old)))
    k, a, d = [], [], []
    for c, rows in CLASS_ROWS.items():
        for val, diff in rows:
            sel = keys[classes == c]
            k.append(sel)
            a.append(np.full(len(sel), val))
            d.append(np.full(len(sel), diff))
    k, a, d = (np.concatenate(x) for x in (k, a, d))
    p = rng.permutation(len(k))
    return state, (k[p], a[p], np.ones(len(k)), d[p])


def split(rows, how, rng):
    """The push as two streams for reduce_push2."""
    n = len(rows[0])
    if how == "first_empty":
        return EMPTY, rows
    if how == "second_empty":
        return rows, EMPTY
    left = rng.random(n) < 0.5
    return (tuple(np.asarray(c)[left] for c in rows),
            tuple(np.asarray(c)[~left] for c in rows))


def oracle_outputs(o, pushes):
    """The oracle's SUM + COUNT reduce over the concatenated streams."""
    oop = o.reduce_create(spec_of("plain"))
    return [o.reduce_push(oop, upd(cat(*s), lo, up)) for s, lo, up in pushes]


def run(g, o, op, pushes, what, want=None):
    """pushes: [(streams, lower, upper)], streams one tuple (reduce_push)
    or two (reduce_push2). Both checks on every push; returns the last
    output's columns. `want`: the expected columns per push when the caller
    has them already, else the oracle's."""
    gop = g.reduce_create(spec_of(op))
    if want is None:
        want = oracle_outputs(o, pushes)
    got = None
    for i, (streams, lo, up) in enumerate(pushes):
        us = [upd(s, lo, up) for s in streams]
        dev = (g.reduce_push_dev(gop, us[0]) if len(us) == 1
               else g.reduce_push2_dev(gop, us[0], us[1]))
        got = dev.to_host()
        dev.release()
        if want[i] is not None:
            vd.assert_cols_equal(got, want[i], f"{what} push {i}: vs oracle")
        again = g.consolidate(abi.schema(1, 48),
                              abi.make_updates(*got, lo, up))
        vd.assert_cols_equal(again, got, f"{what} push {i}: consolidated")
    g.reduce_drop(gop)
    return got


@pytest.mark.parametrize("cls", sorted(CLASS_ROWS))
@pytest.mark.parametrize("op", OPS)
def test_one_group(g, o, op, cls):
    rng = np.random.default_rng(cls)
    # a second key builds the state so that class 0 has a table to miss in
    state, push = state_and_push([cls], rng)
    state = cat(state, (np.array([99]), np.array([10]), np.array([0]),
                        np.array([1])))
    got = run(g, o, op, [((state,), 0, 1), ((push,), 1, 2)], f"class {cls}")
    assert len(got[2]) == ROWS_OUT[cls]
    if cls in (2, 4):    # old row first
        assert got[3].tolist() == [-1, 1]
    if cls == 3:         # new row first
        assert got[3].tolist() == [1, -1]


@pytest.mark.parametrize("path", ["push", "push2"])
@pytest.mark.parametrize("op", OPS)
def test_65_groups(g, o, op, path):
    """More groups than one wave has lanes, all six classes."""
    rng = np.random.default_rng(65)
    classes = np.arange(65) % 6
    state, push = state_and_push(classes, rng)
    streams = (push,) if path == "push" else split(push, "random", rng)
    got = run(g, o, op, [((state,), 0, 1), (streams, 1, 2)], path)
    assert len(got[2]) == sum(ROWS_OUT[c] for c in classes.tolist())


@pytest.mark.parametrize("how", ["first_empty", "second_empty"])
@pytest.mark.parametrize("op", OPS)
def test_push2_one_stream_empty(g, o, op, how):
    rng = np.random.default_rng(7)
    state, push = state_and_push(np.arange(30) % 6, rng)
    got = run(g, o, op, [((state,), 0, 1), (split(push, how, rng), 1, 2)],
              how)
    assert len(got[2]) == 5 * sum(ROWS_OUT.values())


@pytest.mark.parametrize("op", OPS)
def test_push2_both_streams_empty(g, o, op):
    rng = np.random.default_rng(8)
    state, _ = state_and_push(np.arange(12) % 6, rng)
    got = run(g, o, op, [((state,), 0, 1), ((EMPTY, EMPTY), 1, 2)], "empty")
    assert len(got[2]) == 0


@pytest.fixture(scope="module")
def big(o):
    """2048 * 256 + 7 groups, computed once for both operators. Every key
    of a class emits the same rows but for the key, so the expected columns
    are the oracle's output for six keys, one per class, laid out per key
    (the oracle itself takes several seconds at this size)."""
    rng = np.random.default_rng(9)
    six = [((s,), t, t + 1) for t, s in
           enumerate(state_and_push(np.arange(6), rng))]
    _, (k6, v6, t6, d6) = oracle_outputs(o, six)
    assert len(t6) == sum(ROWS_OUT.values())
    v6 = np.asarray(v6, np.uint8).reshape(len(t6), 48)
    classes = np.arange(GRID_CAP_GROUPS + 7) % 6
    keys = np.arange(len(classes), dtype=np.int64) - len(classes) // 2
    counts = np.array([ROWS_OUT[c] for c in range(6)])[classes]
    first = np.cumsum(counts) - counts
    n = int(counts.sum())
    vals, diffs = np.zeros((n, 48), np.uint8), np.zeros(n, np.int64)
    at6 = 0
    for c in range(6):  # the oracle's six keys are in class order
        for j in range(ROWS_OUT[c]):
            vals[first[classes == c] + j] = v6[at6]
            diffs[first[classes == c] + j] = np.asarray(d6)[at6]
            at6 += 1
    want = (np.repeat(keys, counts), vals.ravel(), np.ones(n, np.uint64),
            diffs)
    state, push = state_and_push(classes, rng)
    pushes = [((state,), 0, 1), (split(push, "random", rng), 1, 2)]
    return pushes, want


@pytest.mark.parametrize("op", OPS)
def test_more_groups_than_the_grid(g, o, op, big):
    """The apply and compaction kernels' grid-stride loops take a second
    iteration. Through reduce_push2, both streams non-empty."""
    pushes, want = big
    got = run(g, o, op, pushes, "grid cap", want=[None, want])
    assert len(got[2]) == len(want[2]) > GRID_CAP_GROUPS


@pytest.mark.parametrize("op", OPS)
def test_multi_time_push_keeps_the_sorted_path(g, o, op):
    """upper = lower + 3 with three distinct times in one push: created at
    t, changed at t + 1, half deleted at t + 2. The canonical order is
    key-major across the times, which only the retained sort restores."""
    n = 200
    rng = np.random.default_rng(10)
    keys = np.arange(n, dtype=np.int64) - 77
    half = keys[::2]
    rows = cat((keys, np.full(n, 10), np.full(n, 4), np.ones(n)),
               (keys, np.full(n, 10), np.full(n, 5), -np.ones(n)),
               (keys, np.full(n, -25), np.full(n, 5), np.ones(n)),
               (half, np.full(len(half), -25), np.full(len(half), 6),
                -np.ones(len(half))))
    p = rng.permutation(len(rows[0]))
    rows = tuple(c[p] for c in rows)
    got = run(g, o, op, [((rows,), 4, 7)], "multi-time")
    assert len(got[2]) == n + 2 * n + len(half)
    assert sorted(set(got[2].tolist())) == [4, 5, 6]
