"""Overflow relaunch of the probe protocol. A probe sizes
its ok queue at cap = (hint + 1) * n + 1024 rows (hint 1 on an
arrangement's first probe, so 2n + 1024) and its error queue at
ecap = n / 4 + 1024; the varlen probe's byte queue holds 64 * cap. A launch
whose exact counts exceed either queue is repeated once at the exact
counts. Each case here is shaped to overflow one named queue on a fresh
arrangement, compares the result with the CPU oracle, and, where the
engine counts probe launches, asserts which path ran: two launches on
the first call, one on the repeat (the hint has caught up)."""
import os

import numpy as np
import pytest

from materialize_amd import _abi as abi
from pyoracle_vl import VlOracle
from test_err_stream import _cl_div, _consolidate_host
from test_varlen import _mk_updates

pytestmark = pytest.mark.gpu

VARLEN = abi.MZ_GPU_VARLEN
N = 64        # delta rows: cap = 2 * 64 + 1024 = 1152, ecap = 1040
FAN = 40      # lookup vals per key: 64 * 40 = 2560 matches


def _i64_cols(*cols):
    """Pack int64 columns side by side into an (n, 8 * len(cols)) val."""
    n = len(cols[0])
    v = np.zeros((n, 8 * len(cols)), np.uint8)
    for c, col in enumerate(cols):
        v[:, 8 * c:8 * c + 8] = np.asarray(col, np.int64) \
            .reshape(-1, 1).view(np.uint8).reshape(n, 8)
    return v


def _fanout_updates(n_keys, fan, val_cols, t=0):
    """n_keys ascending keys, `fan` rows each; val_cols(keys, j) -> val."""
    keys = np.repeat(np.arange(n_keys, dtype=np.int64), fan)
    j = np.tile(np.arange(fan, dtype=np.int64), n_keys)
    n = len(keys)
    return abi.make_updates(keys, val_cols(keys, j), np.full(n, t, np.uint64),
                            np.ones(n, np.int64), t, t + 1)


def _delta(n, t, vb=8, sorted=0):
    keys = np.arange(n, dtype=np.int64)
    vals = _i64_cols(keys * 7 + 100) if vb else None
    diffs = np.where(keys % 3 == 0, -1, 1).astype(np.int64)
    return abi.make_updates(keys, vals, np.full(n, t, np.uint64), diffs, t,
                            t + 1, sorted=sorted)


def _cl_pair():
    return abi.closure(
        [], [abi.field(abi.MZ_SRC_KEY, 0, 8)],
        [abi.field(abi.MZ_SRC_VAL_STREAM, 0, 8),
         abi.field(abi.MZ_SRC_VAL_LOOKUP, 0, 8)],
        abi.schema(1, 16))


def _launches(g, call):
    """Run call() and return (result, probe launches it made).
    probe_stats() hands back the counters accumulated since its last
    read, so the read before the call opens the interval."""
    g.probe_stats()
    res = call()
    return res, g.probe_stats()[2]


def _assert_cols(got, want, what):
    for x, y, col in zip(got, want, ("keys", "vals", "times", "diffs")):
        np.testing.assert_array_equal(np.asarray(x).view(np.uint8),
                                      np.asarray(y).view(np.uint8),
                                      err_msg=f"{what} {col}")


def _assert_errs(got, want):
    for x, y, col in zip(got, want, ("codes", "times", "diffs")):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y),
                                      err_msg=f"err {col}")


def _ctxs():
    from materialize_amd._ffi import GpuCtx
    from pyoracle import OracleCtx
    g, o = GpuCtx(), OracleCtx()
    g.set_kernel_timing(True)
    return g, o


def test_ok_queue_overflow_hash_walk():
    """64 delta rows x 40 vals per key: M = 2560 > cap = 1152."""
    g, o = _ctxs()
    sch = abi.schema(1, 8)
    ga, oa = g.arr_create(sch), o.arr_create(sch)
    u = _fanout_updates(N, FAN, lambda k, j: _i64_cols(k * 1000 + j))
    g.arr_insert(ga, u)
    o.arr_insert(oa, u)
    d, cl = _delta(N, 1), _cl_pair()
    want = o.halfjoin(oa, d, 8, True, cl)
    assert len(want[2]) == N * FAN
    first, l1 = _launches(g, lambda: g.halfjoin(ga, d, 8, True, cl))
    _assert_cols(first, want, "first")
    assert l1 == 2, "first probe must overflow the ok queue and relaunch"
    again, l2 = _launches(g, lambda: g.halfjoin(ga, d, 8, True, cl))
    _assert_cols(again, want, "repeat")
    assert l2 == 1, "the repeat is sized from the hint (40): one launch"
    g.close()
    o.close()


def test_ok_queue_overflow_join_push_swapped():
    """The same overflow through the linear join with the delta as input
    2 (swap = 1: the closure's v1 is the lookup val)."""
    g, o = _ctxs()
    sch = abi.schema(1, 8)
    ga1, ga2 = g.arr_create(sch), g.arr_create(sch)
    oa1, oa2 = o.arr_create(sch), o.arr_create(sch)
    u = _fanout_updates(N, FAN, lambda k, j: _i64_cols(k * 1000 + j))
    g.arr_insert(ga1, u)
    o.arr_insert(oa1, u)
    cl = _cl_pair()
    gop, oop = g.join_create(ga1, ga2, cl), o.join_create(oa1, oa2, cl)
    d = _delta(N, 1)
    want = o.join_push(oop, 2, d)
    assert len(want[2]) == N * FAN
    got, l1 = _launches(g, lambda: g.join_push(gop, 2, d))
    _assert_cols(got, want, "join side 2")
    assert l1 == 2
    g.close()
    o.close()


def test_err_queue_overflow():
    """Every lookup divisor is zero: M = 0, E = 2560 > ecap = 1040. The
    lookup val is (divisor = 0, j): the second word keeps the 40 vals of
    a key distinct, the closure reads only the first."""
    g, o = _ctxs()
    sch = abi.schema(1, 16)
    ga, oa = g.arr_create(sch), o.arr_create(sch)
    u = _fanout_updates(N, FAN, lambda k, j: _i64_cols(np.zeros_like(j), j))
    g.arr_insert(ga, u)
    o.arr_insert(oa, u)
    d, cl = _delta(N, 1), _cl_div()
    want = o.halfjoin(oa, d, 8, True, cl)
    want_errs = o.last_errs
    assert len(want[2]) == 0 and len(want_errs[0]) > 0
    got, l1 = _launches(g, lambda: g.halfjoin(ga, d, 8, True, cl))
    got_errs = g.last_errs
    assert len(got[2]) == 0, "ok stream must be empty"
    _assert_cols(got, want, "ok")
    _assert_errs(got_errs, want_errs)
    assert l1 == 2, "E = 2560 must overflow the error queue and relaunch"
    g.close()
    o.close()


@pytest.mark.parametrize("zero_quarter", [False, True],
                         ids=["ok_only", "ok_and_err"])
def test_fused_path_overflow(zero_quarter):
    """halfjoin2 with fan-out 8 per stage over 64 rows: 4096 final rows
    > cap = 1152. With a quarter of the stage-2 divisors zero, 3072 ok
    rows and 1024 error rows both travel through the relaunch."""
    g, o = _ctxs()
    F = 8
    # stage 1: lookup val = (k2, carry); stage 2: carry / divisor(k2)
    cl1 = abi.closure(
        [], [abi.field(abi.MZ_SRC_VAL_LOOKUP, 0, 8)],
        [abi.field(abi.MZ_SRC_VAL_LOOKUP, 8, 8)], abi.schema(1, 8))
    cl2 = _cl_div()
    u1 = _fanout_updates(N, F, lambda k, j: _i64_cols(j, k * F + j + 1))
    # stage-2 val = (divisor, j): divisors 1..8, or 0 where j % 4 == 0
    u2 = _fanout_updates(
        F, F, lambda k, j: _i64_cols(
            np.where(j % 4 == 0, 0, j + 1) if zero_quarter else j + 1, j))

    def build(ctx):
        a1, a2 = (ctx.arr_create(abi.schema(1, 16)),
                  ctx.arr_create(abi.schema(1, 16)))
        ctx.arr_insert(a1, u1)
        ctx.arr_insert(a2, u2)
        return a1, a2

    ga1, ga2 = build(g)
    oa1, oa2 = build(o)
    d = _delta(N, 1, vb=0)
    # reference: the two-call sequence on the oracle
    s1k, s1v, s1t, s1d = o.halfjoin(oa1, d, 0, True, cl1)
    u_mid = abi.make_updates(np.asarray(s1k, np.int64).reshape(-1),
                             np.asarray(s1v, np.uint8),
                             np.asarray(s1t, np.uint64),
                             np.asarray(s1d, np.int64), 1, 2)
    s2 = o.halfjoin(oa2, u_mid, 8, True, cl2)
    want_errs = o.last_errs
    want = _consolidate_host(*s2)
    n_err = N * F * F // 4 if zero_quarter else 0
    assert (len(want_errs[0]) > 0) == zero_quarter

    def fused():
        out = g.halfjoin2_dev(ga1, True, cl1, ga2, True, cl2, d, 0)
        cols, errs = out.to_host(), out.errs_to_host()
        out.release()
        return cols, errs

    for expect in (2, 1):  # overflow + relaunch, then sized from the hint
        (cols, errs), launches = _launches(g, fused)
        assert len(cols[2]) == N * F * F - n_err  # raw rows, one per match
        assert _consolidate_host(*cols) == want
        _assert_errs(errs, want_errs)
        assert launches == expect
    g.close()
    o.close()


def _vl_case(n, fan, val_len):
    """n ascending keys x `fan` distinct vals of val_len bytes at time 0,
    probed by one delta row per key at time 1 (le)."""
    from materialize_amd._ffi import GpuCtx
    g, o = GpuCtx(), VlOracle()
    garr = g.arr_create(abi.schema(1, VARLEN))
    oarr = o.arr_create(1)
    keys = np.repeat(np.arange(n, dtype=np.int64), fan)
    rows = len(keys)
    vals = [bytes([i % 251, (i // 251) % 251]) + bytes(val_len - 2)
            for i in range(rows)]
    times, diffs = np.zeros(rows, np.uint64), np.ones(rows, np.int64)
    u, (arena, offs) = _mk_updates(keys, vals, times, diffs, 0, 1)
    g.arr_insert(garr, u)
    o.arr_insert(oarr, keys.view(np.uint64), 1, arena, offs, times, diffs)
    cl = abi.closure(
        [], [abi.field(abi.MZ_SRC_KEY, 0, 8)],
        [abi.field(abi.MZ_SRC_VAL_LOOKUP, 0, 0)],  # whole-val passthrough
        abi.Schema(key_words=1, val_bytes=VARLEN))
    pk = np.arange(n, dtype=np.int64)
    pt = np.full(n, 1, np.uint64)
    pd = np.where(pk % 3 == 0, -1, 1).astype(np.int64)
    gk, garena, gt, gd = g.halfjoin(
        garr, abi.make_updates(pk, None, pt, pd, 1, 2), 0, True, cl)
    goffs = g.last_voffs
    ok, oarena, ooffs, ot, od = o.halfjoin(oarr, pk.view(np.uint64), 1, pt,
                                           pd, True)
    assert len(ot) == n * fan and len(oarena) == n * fan * val_len
    for x, y, what in ((gk, ok, "keys"), (goffs, ooffs, "offs"),
                       (garena, oarena, "arena"), (gt, ot, "times"),
                       (gd, od, "diffs")):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y),
                                      err_msg=what)
    g.close()


def test_varlen_row_overflow():
    """64 x 40 = 2560 rows > cap = 1152 (bytes fit: 20480 <= 73728)."""
    _vl_case(64, 40, 8)


def test_varlen_byte_overflow_only():
    """32 x 30 = 960 rows <= cap = 1088, but 96000 bytes > 64 * 1088 =
    69632: only the byte queue overflows."""
    _vl_case(32, 30, 100)


def test_merge_scan_and_walk_share_queue_overflow():
    """A sorted delta against a two-batch spine with the merge scan
    forced on: the 4096-key batch is eligible for it (sorted delta,
    >= 4096 keys, threshold 0), the 100-key batch is not and takes the
    hash walk, so both kernels emit into one queue. 512 rows x 8 vals =
    4096 matches > cap = 2 * 512 + 1024. The engine does not report which
    kernel probed a batch; the assertions are parity and the relaunch."""
    g, o = _ctxs()
    sch = abi.schema(1, 8)
    ga, oa = g.arr_create(sch), o.arr_create(sch)
    big = _fanout_updates(4096, 8, lambda k, j: _i64_cols(k * 8 + j))
    small = _fanout_updates(100, 1, lambda k, j: _i64_cols(-k - 1), t=1)
    for u in (big, small):
        g.arr_insert(ga, u)
        o.arr_insert(oa, u)
    assert g.arr_stats(ga)[0] == 2, "the spine must hold two batches"
    d, cl = _delta(512, 2, sorted=1), _cl_pair()
    want = o.halfjoin(oa, d, 8, True, cl)
    assert len(want[2]) == 512 * 8 + 100
    saved = {k: os.environ.get(k)
             for k in ("MZ_PROBE_MERGE", "MZ_PROBE_MERGE_MIN_MB")}
    os.environ["MZ_PROBE_MERGE"] = "1"
    os.environ["MZ_PROBE_MERGE_MIN_MB"] = "0"
    try:
        got, launches = _launches(g, lambda: g.halfjoin(ga, d, 8, True, cl))
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    _assert_cols(got, want, "merge + walk")
    assert launches == 2
    g.close()
    o.close()
