"""arr_flush_take hands the pending insert's consolidated rows over as an
out-batch that owns its four columns. The lane writes the hand-off's times
and diffs while it consolidates (the emit kernel writes them beside the
batch's own), so the flush synchronises once and copies nothing.

Checked here: the rows taken; that they outlive the batch they came from;
that an insert which cancels to nothing hands over nothing and leaks
nothing; and the redo after a cached sort plan did not cover the batch."""
import numpy as np
import pytest

import valdomain as vd
from materialize_amd import _abi as abi
from test_sort_plan_gpu import _dev_updates

pytestmark = pytest.mark.gpu

SCH = (1, 8)


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


def pool_used_bytes():
    """Bytes this process holds in the device's default memory pool, which
    every owned column of the library comes from (hipMallocAsync). Asked of
    the HIP runtime the process already has loaded."""
    import ctypes as C
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    pool, used = C.c_void_p(), C.c_uint64()
    assert hip.hipDeviceGetDefaultMemPool(C.byref(pool), 0) == 0
    USED_MEM_CURRENT = 7  # hipMemPoolAttrUsedMemCurrent
    assert hip.hipMemPoolGetAttribute(pool, USED_MEM_CURRENT,
                                      C.byref(used)) == 0
    return used.value


def churn(rng, n, t, klo=0, khi=400, vlo=0, vhi=6):
    """n rows over few keys and vals at time t: many duplicates, some of
    which cancel."""
    keys = rng.integers(klo, khi, (n, 1)).astype(np.int64)
    vals = rng.integers(vlo, vhi, n).astype(np.int64) \
        .view(np.uint8).reshape(n, 8).copy()
    return (keys, vals, np.full(n, t, np.uint64),
            rng.choice(np.array([-1, 1, 1, 2], np.int64), n))


def insert_take(g, ga, batch, t, keep):
    """Device-staged async insert, then flush_take."""
    keys, vals, times, diffs = batch
    du, refs = _dev_updates(keys, vals, times.view(np.int64), diffs, t, t + 1)
    keep.append(refs)  # device inputs must outlive the flush
    g.arr_insert_async(ga, du)
    return g.arr_flush_take(ga)


def assert_taken(took, o, batch, t, what):
    want = o.consolidate(abi.schema(*SCH), vd.updates(abi, batch, t, t + 1))
    got = took.to_host()
    assert vd.to_rows(*got, *SCH) == vd.naive_consolidated(batch, *SCH), \
        f"{what}: vs naive"
    vd.assert_cols_equal(got, want, f"{what}: vs oracle")


def test_taken_rows_outlive_their_batch(g, o):
    """Take a batch, then insert until arr_maintain merges the spine into
    one batch, which frees the batch the rows came from, and go on
    inserting so that the freed blocks are handed out again."""
    rng = np.random.default_rng(1)
    ga = g.arr_create(abi.schema(*SCH))
    keep = []
    first = churn(rng, 5000, 0)
    took = insert_take(g, ga, first, 0, keep)
    assert_taken(took, o, first, 0, "fresh")
    others = []
    for t in range(1, 4):
        b = churn(rng, 5000, t)
        others.append((insert_take(g, ga, b, t, keep), b, t))
    g.arr_maintain(ga)
    assert g.arr_stats(ga)[0] == 1
    for t in range(4, 7):
        b = churn(rng, 5000, t)
        others.append((insert_take(g, ga, b, t, keep), b, t))
    assert_taken(took, o, first, 0, "after the merge")
    took.release()
    for tk, b, t in others:
        assert_taken(tk, o, b, t, f"t={t}")
        tk.release()
    got = g.peek_scan(ga, 6, allow_negative=True)
    assert vd.to_rows(*got, *SCH) == \
        vd.naive_as_of([first] + [b for _, b, _ in others], 6, *SCH)


def test_cancelled_insert_takes_nothing_and_leaks_nothing(g):
    """An insert whose rows cancel hands over no out-batch. Its hand-off
    columns (16 bytes per input row) must be freed: were they leaked, the
    last 40 of 50 rounds of 400000 rows would add 256 MB to what the
    process holds in the memory pool; it must not grow by even half of
    that."""
    n = 200_000
    rng = np.random.default_rng(2)
    ga = g.arr_create(abi.schema(*SCH))
    k, v, tm, d = churn(rng, n, 0, khi=50_000)
    d = np.abs(d)
    batch = (np.concatenate([k, k]), np.concatenate([v, v]),
             np.concatenate([tm, tm]), np.concatenate([d, -d]))
    used_at = {}
    for r in range(50):
        keep = []
        assert insert_take(g, ga, batch, 0, keep) is None
        g.lib.mz_gpu_sync(g.ctx)
        if r in (9, 49):
            used_at[r] = pool_used_bytes()
    assert g.arr_stats(ga)[1] == 0
    leaked_would_be = 40 * 16 * 2 * n
    assert used_at[49] - used_at[9] < leaked_would_be // 2


def test_take_after_the_sort_plan_is_tripped(g, o):
    """The first batch primes the cached plan on narrow ranges; the second
    lies far outside them, so its first build is discarded at the flush and
    redone. Both takes, and a third inside the re-primed plan, must be
    right."""
    rng = np.random.default_rng(3)
    ga = g.arr_create(abi.schema(*SCH))
    keep = []
    shapes = [dict(klo=0, khi=400, vlo=0, vhi=6),
              dict(klo=-2**40, khi=2**40, vlo=-2**30, vhi=2**30),
              dict(klo=-2**39, khi=2**39, vlo=-2**29, vhi=2**29)]
    batches = [churn(rng, 3000, t, **s) for t, s in enumerate(shapes)]
    spans = [vd.column_spans(b, *SCH) for b in batches]
    assert not vd.covered(vd.pad_spans(spans[0]), spans[1])
    assert vd.covered(vd.pad_spans(spans[1]), spans[2])
    for t, b in enumerate(batches):
        took = insert_take(g, ga, b, t, keep)
        assert_taken(took, o, b, t, f"batch {t}")
        took.release()
    got = g.peek_scan(ga, 2, allow_negative=True)
    assert vd.to_rows(*got, *SCH) == vd.naive_as_of(batches, 2, *SCH)
