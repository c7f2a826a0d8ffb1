"""The seal chain behind arr_insert: sort (identity written by the first
sort-key kernel, final permutation landing in the caller's buffer for odd
and even chunk counts), consolidation, and the batch build over ONE packed
key-id | val-id scan. Each arrangement is read back whole (peek_scan) and
probed (halfjoin); both must equal the naive consolidation of what went
in."""
import numpy as np
import pytest

import valdomain as vd
from materialize_amd import _abi as abi

pytestmark = pytest.mark.gpu

T_READ = 9  # every case's times are below this


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


def i64_vals(x):
    x = np.ascontiguousarray(x, np.int64)
    return x.view(np.uint8).reshape(len(x), 8).copy()


def check_arrangement(g, batch, kw, what):
    """Insert `batch` (vb = 8) into a fresh arrangement; the full read and
    a halfjoin of every key (plus one absent) must match the naive
    reference. Returns the rows read."""
    sch = abi.schema(kw, 8)
    ga = g.arr_create(sch)
    g.arr_insert(ga, vd.updates(abi, batch, 0, T_READ))
    want = vd.naive_as_of([batch], T_READ, kw, 8)
    got = g.peek_scan(ga, T_READ, allow_negative=True)
    assert vd.to_rows(*got, kw, 8) == want, f"{what}: full read"
    assert g.arr_stats(ga)[1] == len(vd.naive_consolidated(batch, kw, 8)), \
        f"{what}: rows held"
    pk = np.unique(np.concatenate([batch[0], np.full((1, kw), 12345)]), axis=0)
    n = len(pk)
    stream = (pk, np.zeros((n, 0), np.uint8),
              np.full(n, T_READ, np.uint64), np.ones(n, np.int64))
    su = vd.updates(abi, stream, T_READ, T_READ + 1)
    for le in (True, False):
        got_j = g.halfjoin(ga, su, 0, le, vd.probe_closure(abi, kw))
        assert vd.to_rows(*got_j, kw, 8) == \
            vd.naive_halfjoin(stream, [batch], kw, le), f"{what}: le={le}"
    return want


def test_one_row(g):
    b = (np.array([[-7]], np.int64), i64_vals([3]), np.array([2], np.uint64),
         np.array([5], np.int64))
    assert check_arrangement(g, b, 1, "one row") == [((-7,), (3,), T_READ, 5)]


def test_one_key_distinct_vals(g):
    """One key word change, n val changes: kv_off = [0, n]."""
    n = 700
    rng = np.random.default_rng(1)
    b = (np.full((n, 1), 4, np.int64), i64_vals(rng.permutation(n) - 300),
         np.full(n, 1, np.uint64), np.ones(n, np.int64))
    assert len(check_arrangement(g, b, 1, "one key")) == n


def test_one_key_val_distinct_times(g):
    """One key, one val, n updates: vu_off = [0, n]."""
    n = 600
    rng = np.random.default_rng(2)
    b = (np.full((n, 1), 4, np.int64), i64_vals(np.full(n, -1)),
         (rng.permutation(n) % T_READ).astype(np.uint64),
         np.ones(n, np.int64))
    sch = abi.schema(1, 8)
    ga = g.arr_create(sch)
    g.arr_insert(ga, vd.updates(abi, b, 0, T_READ))
    assert g.arr_stats(ga)[1] == len(np.unique(b[2]))  # a row per time
    assert check_arrangement(g, b, 1, "one val") == [((4,), (2**64 - 1,),
                                                      T_READ, n)]


def test_batch_cancels_to_nothing(g):
    n = 500
    rng = np.random.default_rng(3)
    k = rng.integers(-50, 50, (n, 1)).astype(np.int64)
    v = i64_vals(rng.integers(0, 3, n))
    t = rng.integers(0, 4, n).astype(np.uint64)
    d = rng.integers(1, 4, n).astype(np.int64)
    p = rng.permutation(2 * n)
    b = (np.concatenate([k, k])[p], np.concatenate([v, v])[p],
         np.concatenate([t, t])[p], np.concatenate([d, -d])[p])
    assert check_arrangement(g, b, 1, "cancels") == []


def wide_batch(rng, n, kw, tspan):
    """Full-width key words and val word; times constant (tspan = 0) or a
    few bits wide, which makes the time a chunk of its own in front of the
    64-bit val word."""
    keys, vals, _, diffs = vd.gen_full(rng, n, kw, 8)
    times = np.uint64(2) + rng.integers(0, tspan + 1, n, dtype=np.uint64)
    times[0], times[1] = 2, 2 + tspan
    return keys, vals, times, diffs


@pytest.mark.parametrize("chunks,kw,tspan", [(2, 1, 0), (3, 1, 4), (3, 2, 0),
                                             (4, 2, 4)])
def test_sort_chunk_parity_full_width(g, chunks, kw, tspan):
    """Odd and even numbers of radix sorts: the permutation ping-pongs
    between two buffers and must end in the one consolidation reads."""
    b = wide_batch(np.random.default_rng(10 * kw + tspan), 1500, kw, tspan)
    assert len(vd.plan_shape(b, kw, 8)) == chunks
    check_arrangement(g, b, kw, f"{chunks} chunks")


def test_sort_one_chunk(g):
    b = vd.gen_narrow(np.random.default_rng(5), 1500, 1, 8)
    b[2][:] = b[2] - np.uint64(2**63)  # times 0..4
    assert len(vd.plan_shape(b, 1, 8)) == 1
    check_arrangement(g, b, 1, "1 chunk")


def test_sort_zero_chunks(g):
    """Every column constant: no sort runs, and consolidation still needs
    the identity permutation."""
    n = 1000
    b = (np.full((n, 1), -2**63, np.int64), i64_vals(np.full(n, 2**63 - 1)),
         np.full(n, 3, np.uint64), np.full(n, 2, np.int64))
    assert vd.plan_shape(b, 1, 8) == []
    assert check_arrangement(g, b, 1, "constant") == \
        [((-2**63,), (2**63 - 1,), T_READ, 2 * n)]
