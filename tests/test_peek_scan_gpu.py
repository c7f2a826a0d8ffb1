"""Full-scan peek (mz_gpu_peek_scan / k_scan_walk) on the GPU.

Reference: a naive recompute (scan_ref below) — concatenate every update
ever inserted, keep time <= as_of, apply the closure in Python, group by
(key words, val bytes) with wrapping i64 sums, drop zeros, sort in the
engine's canonical order (keys as signed tuples, vals as little-endian u64
words, the last one zero-padded). All four output columns are compared
byte for byte. Second reference: the keyed peek over all distinct keys,
which is held to the oracle elsewhere.
"""
import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd.tpch import TpchGen
from materialize_amd.workloads import Q3Dataflow

pytestmark = pytest.mark.gpu

KEY, VL, CP = abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_LOOKUP, abi.MZ_SRC_COMPUTE
F, FL = abi.field, abi.filt
ERR = "err"


# ------------------------------------------------------------ reference

def wrap(d):
    return ((d + 2**63) % 2**64) - 2**63


def i64_at(v, off):
    return int.from_bytes(v[off:off + 8], "little", signed=True)


def i64_bytes(x):
    return wrap(x).to_bytes(8, "little", signed=True)


def val_words(v):
    return tuple(int.from_bytes(v[o:o + 8], "little")
                 for o in range(0, len(v), 8))


def scan_ref(batches, as_of, fn=None):
    """batches: (keys[n, kw] i64, vals[n, vb] u8, times[n], diffs[n]) per
    insert. fn(key tuple, val bytes) -> None (filtered) | ERR | (out key
    tuple, out val bytes). Returns ((keys, vals, times, diffs), err sum)."""
    acc, err = {}, 0
    for keys, vals, times, diffs in batches:
        for i in range(len(times)):
            if int(times[i]) > as_of:
                continue
            row = (tuple(int(x) for x in keys[i]), vals[i].tobytes())
            if fn is not None:
                row = fn(*row)
            if row is None:
                continue
            if row == ERR:
                err = wrap(err + int(diffs[i]))
                continue
            acc[row] = wrap(acc.get(row, 0) + int(diffs[i]))
    rows = sorted(((k, v, d) for (k, v), d in acc.items() if d != 0),
                  key=lambda r: (r[0], val_words(r[1])))
    n = len(rows)
    keys = np.array([x for r in rows for x in r[0]], np.int64)
    vals = np.frombuffer(b"".join(r[1] for r in rows), np.uint8)
    return ((keys, vals, np.full(n, as_of, np.uint64),
             np.array([r[2] for r in rows], np.int64)), err)


def same(got, want, what):
    for a, b, col in zip(got, want, ("keys", "vals", "times", "diffs")):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype.itemsize == b.dtype.itemsize, f"{what}: {col} dtype"
        np.testing.assert_array_equal(
            np.ascontiguousarray(a).view(np.uint8),
            np.ascontiguousarray(b).view(np.uint8), err_msg=f"{what}: {col}")


def check(g, arr, batches, as_of, mfp=None, fn=None, what="", **kw):
    want, err = scan_ref(batches, as_of, fn)
    got = g.peek_scan(arr, as_of, mfp, **kw)
    same(got, want, f"{what} as_of={as_of}")
    ecodes, etimes, ediffs = g.last_errs
    if err == 0:
        assert len(ecodes) == 0, f"{what}: unexpected error rows"
    else:  # one consolidated (code, as_of, sum) row
        assert ecodes.tolist() == [abi.MZ_ERR_DIVISION_BY_ZERO]
        assert etimes.tolist() == [as_of] and ediffs.tolist() == [err]
    return got


def upd(batch, lower, upper):
    keys, vals, times, diffs = batch
    return abi.make_updates(keys.ravel(),
                            vals.ravel() if vals.shape[1] else None,
                            times, diffs, lower, upper)


def build(g, kw, vb, batches, bounds):
    arr = g.arr_create(abi.schema(kw, vb))
    for b, (lo, hi) in zip(batches, bounds):
        g.arr_insert(arr, upd(b, lo, hi))
    return arr


def ab_vals(a, b):
    """16-byte vals [a i64][b i64]."""
    return np.stack([a, b], 1).astype(np.int64).view(np.uint8) \
        .reshape(len(a), 16)


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


# ------------------------------------------- wave tails, uniform reserve

MFP_THIRD = abi.closure([FL(VL, 8, 8, abi.MZ_CMP_EQ, 0)],
                        [F(KEY, 0, 8)], [F(VL, 0, 16)], abi.schema(1, 16))


def fn_third(k, v):
    return (k, v) if i64_at(v, 8) == 0 else None


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_wave_tails(g, n):
    """One batch of exactly n vals; the filter keeps every third, so lanes
    with nothing to emit sit beside lanes that emit, and the last wave is
    partly idle. Times alternate 0/1: as_of 0 reads the time column, as_of
    1 is the allpass case."""
    i = np.arange(n)
    batch = ((i - n // 2).reshape(n, 1).astype(np.int64),
             ab_vals(i * 7, i % 3), (i % 2).astype(np.uint64),
             (1 + i % 2).astype(np.int64))
    arr = build(g, 1, 16, [batch], [(0, 2)])
    assert g.arr_stats(arr)[:2] == (1, n)
    for as_of in (0, 1):
        check(g, arr, [batch], as_of, what=f"n={n} identity")
        check(g, arr, [batch], as_of, MFP_THIRD, fn_third,
              what=f"n={n} every third")


# -------------------------- multiple batches, cancellation, time filter

def _multi_batches():
    """Four inserts at t = 0..3 of 3000 rows: keys < 300, vals < 8, diffs in
    {+1, +1, -1}; a retraction only ever takes back a row whose net count
    from EARLIER times still covers it, so net counts stay >= 0 at every
    time (verified below with the naive model)."""
    rng = np.random.default_rng(20240)
    live, batches = {}, []
    for t in range(4):
        keys, vals, diffs = [], [], []
        # what earlier times left to retract, one entry per copy
        avail = [r for r, c in sorted(live.items()) for _ in range(c)]
        rng.shuffle(avail)
        signs = rng.choice([1, 1, -1], 3000) if t else np.ones(3000, int)
        for s in signs:
            if s < 0 and avail:
                (k, v), d = avail.pop(), -1
            else:
                k, v, d = int(rng.integers(300)), int(rng.integers(8)), 1
            keys.append(k)
            vals.append(v)
            diffs.append(d)
            live[(k, v)] = live.get((k, v), 0) + d
        batches.append((np.array(keys, np.int64).reshape(-1, 1),
                        np.array(vals, np.int64).view(np.uint8)
                        .reshape(-1, 8),
                        np.full(3000, t, np.uint64),
                        np.array(diffs, np.int64)))
    return batches


@pytest.fixture(scope="module")
def multi():
    batches = _multi_batches()
    refs = {}
    for as_of in (0, 1, 2, 3, 10):
        refs[as_of] = scan_ref(batches, as_of)[0]
        assert (refs[as_of][3] > 0).all(), "test data: negative net count"
    assert sum(int((b[3] < 0).sum()) for b in batches) > 1000
    return batches, refs


def _build_multi(g, batches):
    return build(g, 1, 8, batches, [(t, t + 1) for t in range(4)])


def test_multi_batch_time_filter_and_merge(g, multi):
    batches, refs = multi
    arr = _build_multi(g, batches)
    assert g.arr_stats(arr)[0] >= 2
    for as_of in (0, 1, 3, 10):  # 10: every batch allpass
        same(g.peek_scan(arr, as_of), refs[as_of], f"spine as_of={as_of}")
    # one merged batch: a val's update range now holds several times, some
    # beyond as_of
    g.arr_maintain(arr)
    assert g.arr_stats(arr)[0] == 1
    for as_of in (0, 1, 3, 10):
        same(g.peek_scan(arr, as_of), refs[as_of], f"merged as_of={as_of}")


def test_logical_compaction(g, multi):
    from materialize_amd._ffi import MzGpuError
    batches, refs = multi
    arr = _build_multi(g, batches)
    g.arr_set_logical_compaction(arr, 2)
    g.arr_maintain(arr)
    for as_of in (2, 3):
        same(g.peek_scan(arr, as_of), refs[as_of], f"since=2 as_of={as_of}")
    with pytest.raises(MzGpuError, match="compaction frontier"):
        g.peek_scan(arr, 1)


def test_matches_keyed_peek_of_all_keys(g, multi):
    batches, refs = multi
    arr = _build_multi(g, batches)
    allkeys = np.unique(np.concatenate([b[0].ravel() for b in batches]))
    for as_of in (0, 2, 10):
        same(g.peek_scan(arr, as_of), g.peek(arr, allkeys, as_of),
             f"scan vs keyed peek as_of={as_of}")


# ----------------------------------------------------------------- schemas

@pytest.mark.parametrize("kw,vb", [(1, 0), (1, 8), (2, 12), (1, 64)])
def test_schemas(g, kw, vb):
    """500 rows over two batches drawn from a small pool of (key, val)s —
    keys of both signs (key order is signed), val bytes over the whole
    byte range (val order is unsigned little-endian words)."""
    rng = np.random.default_rng(1000 * kw + vb)
    pool_k = rng.integers(-20, 20, (40, kw)).astype(np.int64)
    pool_v = rng.integers(0, 256, (40, vb)).astype(np.uint8)
    batches = []
    for t in range(2):
        pick = rng.integers(0, 40, 250)
        batches.append((pool_k[pick], pool_v[rng.integers(0, 40, 250)],
                        np.full(250, t, np.uint64),
                        rng.integers(1, 4, 250).astype(np.int64)))
    arr = build(g, kw, vb, batches, [(0, 1), (1, 2)])
    assert g.arr_stats(arr)[0] == 2
    for as_of in (0, 1):
        got = check(g, arr, batches, as_of, what=f"schema ({kw},{vb})")
        assert len(got[2]) > 0


# ---------------------------------------------------------- pending insert

def _pending_case(g, flush):
    rng = np.random.default_rng(5)

    def batch(n, t):
        return (rng.integers(-50, 50, (n, 1)).astype(np.int64),
                rng.integers(0, 4, (n, 1)).astype(np.int64).view(np.uint8)
                .reshape(n, 8), np.full(n, t, np.uint64),
                np.ones(n, np.int64))

    b0, b5 = batch(400, 0), batch(300, 5)
    arr = build(g, 1, 8, [b0], [(0, 1)])
    before = g.peek_scan(arr, 4)
    same(before, scan_ref([b0], 4)[0], "before the insert")
    g.arr_insert_async(arr, upd(b5, 5, 6))
    if flush:
        g.arr_flush(arr)
    at4 = g.peek_scan(arr, 4)  # the pending batch lies wholly beyond 4
    at5 = g.peek_scan(arr, 5)  # ... and is part of the answer at 5
    same(at4, before, f"flush={flush}: as_of=4 with a batch at 5 pending")
    same(at5, scan_ref([b0, b5], 5)[0], f"flush={flush}: as_of=5")
    assert len(at5[2]) > len(at4[2])
    return at4, at5


def test_pending_insert(g):
    lazy = _pending_case(g, flush=False)
    flushed = _pending_case(g, flush=True)
    for a, b in zip(lazy, flushed):
        same(a, b, "pending vs flushed")


# ---------------------------------------------------------------- closures

def _closure_batches():
    rng = np.random.default_rng(77)
    out = []
    for t in range(2):
        n = 600
        out.append((rng.integers(-30, 30, (n, 1)).astype(np.int64),
                    ab_vals(rng.integers(-5, 6, n), rng.integers(0, 8, n)),
                    np.full(n, t, np.uint64),
                    rng.integers(1, 3, n).astype(np.int64)))
    return out


CLOSURES = {
    # filter on a val field: b > 3
    "val-filter": (
        abi.closure([FL(VL, 8, 8, abi.MZ_CMP_GT, 3)], [F(KEY, 0, 8)],
                    [F(VL, 0, 16)], abi.schema(1, 16)),
        lambda k, v: (k, v) if i64_at(v, 8) > 3 else None),
    # filter on the key: key >= 0
    "key-filter": (
        abi.closure([FL(KEY, 0, 8, abi.MZ_CMP_GE, 0)], [F(KEY, 0, 8)],
                    [F(VL, 0, 16)], abi.schema(1, 16)),
        lambda k, v: (k, v) if k[0] >= 0 else None),
    # projection dropping a: rows that differ only in a collapse
    "project": (
        abi.closure([], [F(KEY, 0, 8)], [F(VL, 8, 8)], abi.schema(1, 8)),
        lambda k, v: (k, v[8:16])),
    # (a, a * b)
    "mul": (
        abi.closure([], [F(KEY, 0, 8)],
                    [F(VL, 0, 8),
                     F(CP, abi.MZ_COMPUTE_MUL_I64, 8, arg0=0, arg1=8,
                       arg0_src=VL, arg1_src=VL)], abi.schema(1, 16)),
        lambda k, v: (k, v[:8] + i64_bytes(i64_at(v, 0) * i64_at(v, 8)))),
}

# (b, a / b): b == 0 goes to the error stream
MFP_DIV = abi.closure([], [F(KEY, 0, 8)],
                      [F(VL, 8, 8),
                       F(CP, abi.MZ_COMPUTE_DIV_I64, 8, arg0=0, arg1=8,
                         arg0_src=VL, arg1_src=VL)], abi.schema(1, 16))


def fn_div(k, v):
    a, b = i64_at(v, 0), i64_at(v, 8)
    if b == 0:
        return ERR
    q = abs(a) // abs(b)  # C division truncates toward zero
    return k, v[8:16] + i64_bytes(q if (a < 0) == (b < 0) else -q)


@pytest.fixture(scope="module")
def closure_arr(g):
    batches = _closure_batches()
    return build(g, 1, 16, batches, [(0, 1), (1, 2)]), batches


@pytest.mark.parametrize("name", list(CLOSURES))
def test_closures(g, closure_arr, name):
    arr, batches = closure_arr
    mfp, fn = CLOSURES[name]
    for as_of in (0, 1):
        got = check(g, arr, batches, as_of, mfp, fn, what=name)
        assert 0 < len(got[2])
    if name == "project":  # collapsed: fewer rows than the identity scan
        assert len(got[2]) < len(g.peek_scan(arr, 1)[2])


def test_error_stream(g, closure_arr):
    arr, batches = closure_arr
    for as_of in (0, 1):
        want, err = scan_ref(batches, as_of, fn_div)
        assert err > 0 and len(want[2]) > 0
        check(g, arr, batches, as_of, MFP_DIV, fn_div, what="div")


def test_error_queue_overflow_relaunches(g):
    """4200 vals in one batch, every one dividing by zero: 4200 error rows
    exceed the first error queue (4200/4 + 1024 slots), so the exact
    relaunch runs."""
    n = 4200
    i = np.arange(n)
    batch = (i.reshape(n, 1).astype(np.int64), ab_vals(i, np.zeros(n)),
             np.zeros(n, np.uint64), (1 + i % 3).astype(np.int64))
    arr = build(g, 1, 16, [batch], [(0, 1)])
    assert g.arr_stats(arr)[:2] == (1, n)
    assert n > n // 4 + 1024
    g.set_kernel_timing(True)  # the probe statistics count the launches
    try:
        g.probe_stats()
        g.peek_scan(arr, 0)  # no error rows: the first launch holds
        assert g.probe_stats()[1:] == (n, 1)
        got = g.peek_scan(arr, 0, MFP_DIV)
        assert g.probe_stats()[1:] == (n, 2)
    finally:
        g.set_kernel_timing(False)
    assert len(got[2]) == 0 and len(got[0]) == 0
    ecodes, etimes, ediffs = g.last_errs
    assert ecodes.tolist() == [abi.MZ_ERR_DIVISION_BY_ZERO]
    assert etimes.tolist() == [0]
    assert ediffs.tolist() == [int(batch[3].sum())]


# ---------------------------------------------------- negative multiplicity

def _rows(rows):
    """[(key, val, time, diff)] -> a (1, 8) batch."""
    k, v, t, d = zip(*rows)
    return (np.array(k, np.int64).reshape(-1, 1),
            np.array(v, np.int64).view(np.uint8).reshape(-1, 8),
            np.array(t, np.uint64), np.array(d, np.int64))


def test_negative_multiplicity(g, multi):
    from materialize_amd._ffi import MzGpuError
    batch = _rows([(1, 10, 0, 1), (2, 20, 0, -1), (3, 30, 0, 2)])
    arr = build(g, 1, 8, [batch], [(0, 1)])
    with pytest.raises(MzGpuError,
                       match=r"negative multiplicity \(1 rows\)"):
        g.peek_scan(arr, 0)
    got = check(g, arr, [batch], 0, what="allow_negative",
                allow_negative=True)
    assert got[3].tolist() == [1, -1, 2]
    # the failed call left the context usable
    batches, refs = multi
    same(g.peek_scan(_build_multi(g, batches), 3), refs[3],
         "after a failed peek")


def test_sums_wrap(g):
    """2**62 at t=0 and 2**62 at t=1 on one row of one batch: the kernel's
    sum over the val's update range wraps to -2**63."""
    batch = _rows([(7, 1, 0, 2**62), (7, 1, 1, 2**62), (8, 1, 0, 1)])
    arr = build(g, 1, 8, [batch], [(0, 2)])
    assert g.arr_stats(arr)[:2] == (1, 3)
    got = check(g, arr, [batch], 1, what="wrap", allow_negative=True)
    assert got[3].tolist() == [-2**63, 1]
    assert check(g, arr, [batch], 0, what="wrap")[3].tolist() == [2**62, 1]


def test_c_layer_rejects_bad_calls(g, closure_arr):
    """What PeekPlan refuses in Python the ABI entry refuses too, with a
    message and without harming the context."""
    from materialize_amd._ffi import MzGpuError
    arr, batches = closure_arr
    VS = abi.MZ_SRC_VAL_STREAM
    reads_stream = [
        abi.closure([FL(VS, 0, 8, abi.MZ_CMP_EQ, 0)], [F(KEY, 0, 8)],
                    [F(VL, 0, 16)], abi.schema(1, 16)),
        abi.closure([], [F(KEY, 0, 8)], [F(VS, 0, 16)], abi.schema(1, 16)),
        abi.closure([], [F(KEY, 0, 8)],
                    [F(VL, 0, 8),
                     F(CP, abi.MZ_COMPUTE_DIV_I64, 8, arg0=0, arg1=8,
                       arg0_src=VL, arg1_src=VS)], abi.schema(1, 16)),
    ]
    for bad in reads_stream:
        with pytest.raises(MzGpuError, match="MZ_SRC_VAL_STREAM"):
            g.peek_scan(arr, 1, bad)
    with pytest.raises(MzGpuError, match="out schema"):
        g.peek_scan(arr, 1, abi.closure([], [F(KEY, 0, 8)], [F(VL, 0, 8)],
                                        abi.schema(1, 16)))
    for bad in (  # reads beyond the 16 val bytes / the 1 key word
            abi.closure([FL(VL, 12, 8, abi.MZ_CMP_EQ, 0)], [F(KEY, 0, 8)],
                        [F(VL, 0, 16)], abi.schema(1, 16)),
            abi.closure([], [F(KEY, 0, 16)], [F(VL, 0, 16)],
                        abi.schema(2, 16)),
            abi.closure([], [F(KEY, 0, 8)],
                        [F(VL, 0, 8),
                         F(CP, abi.MZ_COMPUTE_MUL_I64, 8, arg0=0, arg1=16,
                           arg0_src=VL, arg1_src=VL)], abi.schema(1, 16))):
        with pytest.raises(MzGpuError, match="reads past"):
            g.peek_scan(arr, 1, bad)
    vl = g.arr_create(abi.schema(1, abi.MZ_GPU_VARLEN))
    with pytest.raises(MzGpuError, match="varlen arrangements unsupported"):
        g.peek_scan(vl, 0)
    check(g, arr, batches, 1, what="after rejected calls")


# ------------------------------------------------------------ empty results

def test_empty_results(g):
    fresh = g.arr_create(abi.schema(1, 8))
    plus, minus = _rows([(1, 10, 0, 1)]), _rows([(1, 10, 1, -1)])
    two = build(g, 1, 8, [plus, minus], [(0, 1), (1, 2)])  # two batches
    both = _rows([(1, 10, 0, 1), (1, 10, 1, -1)])
    one = build(g, 1, 8, [both], [(0, 2)])                 # one val range
    for arr, what in ((fresh, "fresh"), (two, "two batches"),
                      (one, "one batch")):
        k, v, t, d = g.peek_scan(arr, 1)
        assert len(k) == len(v) == len(t) == len(d) == 0, what
        assert len(g.last_errs[0]) == 0, what
    assert g.peek_scan(two, 0)[3].tolist() == [1]
    assert g.peek_scan(one, 0)[3].tolist() == [1]


# -------------------------------------------------------- Q3 view readback

def test_q3_view_readback(g):
    """The Q3 view read back from its output index equals the host-side
    consolidation of every correction the reduce has emitted."""
    df = Q3Dataflow(g, index_output=True)
    captured = []
    orig = df.reduce.push

    def push(u):
        o = orig(u)
        k, v, t, d = o.to_host()
        captured.append((k.reshape(-1, 2), v.reshape(-1, 24), t, d))
        return o

    df.reduce.push = push
    gen = TpchGen(sf=0.01, seed=3)
    df.load(gen)
    assert captured and len(captured[0][2]) > 0
    same(df.peek_result(0), scan_ref(captured, 0)[0], "snapshot")
    at1 = None
    for t in (1, 2, 3):
        _, corr = df.step(gen.churn(2000), t)
        if corr is not None:
            corr.release()
        assert all((c[2] <= t).all() for c in captured)
        want = scan_ref(captured, t)[0]
        same(df.peek_result(t), want, f"step {t}")
        if t == 1:
            at1 = want
    assert len(captured) >= 4
    same(df.peek_result(1), at1, "as of 1 after step 3")
