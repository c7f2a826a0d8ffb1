"""The snapshot-diff push driver under TopK and the window
operator: the paths the operators' own tests reach only by luck.

Every case is tiny (kw = 1, vb = 8, at most 8 groups, 64 rows and three
timestamps): the kernels are the operators' and have their own tests; what
is driven here is the host protocol — slicing, empty snapshots, the
concatenation of several slices against the single slice consolidated in
place, and the clean-up after a slice that fails.

References: OracleCtx.topk_push for TopK; for the window operator the naive
Python model of test_window_agg_gpu.py (test_window_gpu.py's model with the
aggregates added, so that it covers both specs used here).
"""
import numpy as np
import pytest

from materialize_amd import _abi as abi
from test_window_agg_gpu import Rig, i64, updates_of

pytestmark = pytest.mark.gpu

SCH = abi.schema(1, 8)
ORDER = [(0, 8, False)]
WINDOW_SPECS = {
    "row_number": lambda: [abi.wf_row_number()],  # expands
    "sum": lambda: [abi.wf_sum(0, 8)],            # an aggregate, no expansion
}


@pytest.fixture(scope="module")
def ctxs():
    from materialize_amd._ffi import GpuCtx
    from pyoracle import OracleCtx
    g, o = GpuCtx(), OracleCtx()
    yield g, o
    g.close()
    o.close()


def topk_spec():
    return abi.topk_spec(SCH, ORDER, offset=1, limit=2)


def topk_drop(g, op):
    g.lib.mz_gpu_topk_drop(g.ctx, op)


def rows_of(res):
    """(keys, vals, times, diffs) host columns -> sorted [(key, val bytes,
    time, diff)], the multiset of output rows (kw = 1)."""
    k, v, t, d = res
    k = np.asarray(k).view(np.int64).ravel()
    v = np.ascontiguousarray(v).view(np.uint8).ravel()
    vb = len(v) // len(t) if len(t) else 0
    return sorted((int(k[i]), bytes(v[i * vb:(i + 1) * vb]), int(t[i]),
                   int(d[i])) for i in range(len(t)))


def model_rows(want):
    return sorted((r[0][0], r[1], r[2], r[3]) for r in want)


def at(rows, t):
    return [r for r in rows if r[2] == t]


def churn_rows():
    """Six groups, each changed at each of three timestamps, counts never
    negative: 18 + 12 + 12 = 42 rows."""
    rows = []
    for k in range(6):
        rows += [((k,), i64(10 * k + j), 0, 1 + (j + k) % 2)
                 for j in range(3)]
        rows += [((k,), i64(10 * k + 1), 1, -1), ((k,), i64(10 * k - 5), 1, 2)]
        rows += [((k,), i64(10 * k), 2, -(1 + k % 2)),
                 ((k,), i64(10 * k + 7), 2, 1)]
    return rows


# ---------------------------------------------- multi-slice = single-slice

def test_topk_multi_slice_equals_single_slices(ctxs):
    g, o = ctxs
    rows = churn_rows()
    one, ref = g.topk_create(topk_spec()), o.topk_create(topk_spec())
    got = rows_of(g.topk_push(one, updates_of(rows, 8, 0, 3)))
    want = rows_of(o.topk_push(ref, updates_of(rows, 8, 0, 3)))
    three, steps = g.topk_create(topk_spec()), []
    for t in range(3):
        steps += rows_of(g.topk_push(three, updates_of(at(rows, t), 8, t,
                                                       t + 1)))
    assert {r[2] for r in want} == {0, 1, 2}
    assert got == want
    assert sorted(steps) == want
    topk_drop(g, one)
    topk_drop(g, three)


@pytest.mark.parametrize("name", sorted(WINDOW_SPECS))
def test_window_multi_slice_equals_single_slices(ctxs, name):
    g, _ = ctxs
    rows = churn_rows()
    one = Rig(g, SCH, ORDER, WINDOW_SPECS[name]())
    want = model_rows(one.expect(rows))
    got = rows_of(g.window_push(one.op, updates_of(rows, 8, 0, 3)))
    three, steps = Rig(g, SCH, ORDER, WINDOW_SPECS[name]()), []
    for t in range(3):
        steps += rows_of(g.window_push(three.op, updates_of(at(rows, t), 8,
                                                            t, t + 1)))
    assert {r[2] for r in want} == {0, 1, 2}
    assert got == want
    assert sorted(steps) == want
    one.drop()
    three.drop()


# ------------------------------------------------------------ empty sides

def empty_side_rows():
    """Slice 0 creates three groups (no old snapshot), slice 1 changes them,
    slice 2 retracts group 1 completely (no new snapshot for it)."""
    rows = [((k,), i64(v), 0, 1) for k in range(3) for v in (1, 2, 3, 4)]
    rows += [((k,), i64(2), 1, -1) for k in range(3)]
    rows += [((k,), i64(9), 1, 1) for k in range(3)]
    rows += [((1,), i64(v), 2, -1) for v in (1, 3, 4, 9)]
    return rows


# One row inserted and retracted at one time. In group 1, now empty, both
# snapshots are empty and nothing is emitted; in group 0 the two snapshots
# are equal and their rows cancel in the consolidation.
def cancelling(k, t):
    return [((k,), i64(5), t, 1), ((k,), i64(5), t, -1)]


def test_topk_empty_sides(ctxs):
    g, o = ctxs
    rows = empty_side_rows()
    gop, oop = g.topk_create(topk_spec()), o.topk_create(topk_spec())
    got = rows_of(g.topk_push(gop, updates_of(rows, 8, 0, 3)))
    want = rows_of(o.topk_push(oop, updates_of(rows, 8, 0, 3)))
    assert got == want
    # group 1 at time 2: retractions only
    assert [r[3] < 0 for r in got if r[0] == 1 and r[2] == 2] == [True, True]
    for k, t in ((1, 3), (0, 4)):
        u = updates_of(cancelling(k, t), 8, t, t + 1)
        assert rows_of(o.topk_push(oop, u)) == []
        assert len(g.topk_push(gop, u)[2]) == 0
    topk_drop(g, gop)


@pytest.mark.parametrize("name", sorted(WINDOW_SPECS))
def test_window_empty_sides(ctxs, name):
    g, _ = ctxs
    rows = empty_side_rows()
    rig = Rig(g, SCH, ORDER, WINDOW_SPECS[name]())
    want = model_rows(rig.expect(rows))
    got = rows_of(g.window_push(rig.op, updates_of(rows, 8, 0, 3)))
    assert got == want
    gone = [r for r in got if r[0] == 1 and r[2] == 2]
    assert len(gone) == 4 and all(r[3] < 0 for r in gone)
    for k, t in ((1, 3), (0, 4)):
        assert rig.expect(cancelling(k, t)) == []
        u = updates_of(cancelling(k, t), 8, t, t + 1)
        assert len(g.window_push(rig.op, u)[2]) == 0
    rig.drop()


# ------------------------------------------------- failure in a later slice

def failing_rows():
    """Slice 1 retracts more of (group 2, val 1) than slice 0 inserted."""
    rows = [((k,), i64(v), 0, 1) for k in range(4) for v in (1, 2, 3)]
    rows += [((2,), i64(1), 1, -2), ((3,), i64(8), 1, 1)]
    rows += [((k,), i64(6), 2, 1) for k in range(4)]
    return rows


SMALL = [((k,), i64(v), 0, 1) for k in range(3) for v in (4, 1, 3, 2)]


def test_topk_failure_in_a_later_slice(ctxs):
    from materialize_amd._ffi import MzGpuError
    g, o = ctxs
    bad = g.topk_create(topk_spec())
    with pytest.raises(MzGpuError, match="negative multiplicities in TopK"):
        g.topk_push(bad, updates_of(failing_rows(), 8, 0, 3))
    topk_drop(g, bad)
    # the pinned page, the scratch and the allocator are left sound
    gop, oop = g.topk_create(topk_spec()), o.topk_create(topk_spec())
    got = rows_of(g.topk_push(gop, updates_of(SMALL, 8, 0, 1)))
    assert got == rows_of(o.topk_push(oop, updates_of(SMALL, 8, 0, 1)))
    assert len(got) == 6
    topk_drop(g, gop)


@pytest.mark.parametrize("name", sorted(WINDOW_SPECS))
def test_window_failure_in_a_later_slice(ctxs, name):
    from materialize_amd._ffi import MzGpuError
    g, _ = ctxs
    bad = Rig(g, SCH, ORDER, WINDOW_SPECS[name]())
    with pytest.raises(MzGpuError, match="negative multiplicities in window"):
        g.window_push(bad.op, updates_of(failing_rows(), 8, 0, 3))
    bad.drop()
    rig = Rig(g, SCH, ORDER, WINDOW_SPECS[name]())
    want = model_rows(rig.expect(SMALL))
    got = rows_of(g.window_push(rig.op, updates_of(SMALL, 8, 0, 1)))
    assert got == want and len(got) == 12
    rig.drop()
