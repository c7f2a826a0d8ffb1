"""The consolidation chain over a ready permutation: head flag + permuted
diff, one segmented (head, sum) scan, one survivor scan, one emit.

What can go wrong there is positional: a group that starts or ends next to
a 256-thread block or a scan-tile boundary, one group that spans many
tiles, a zero-sum group at either end, a sum that wraps, and the grid cap
(2048 blocks of 256) past which the kernels' grid-stride loops iterate.
Every result is compared row for row, in the order returned, with the naive
tuple reference and byte for byte with the CPU oracle."""
import numpy as np
import pytest

import valdomain as vd
from materialize_amd import _abi as abi

pytestmark = pytest.mark.gpu

GRID_CAP_ROWS = 2048 * 256


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


def check(g, o, kw, vb, batch, what, naive=True):
    sch = abi.schema(kw, vb)
    u = vd.updates(abi, batch, 0, vd.U64_MAX)
    got = g.consolidate(sch, u)
    if naive:
        assert vd.to_rows(*got, kw, vb) == \
            vd.naive_consolidated(batch, kw, vb), f"{what}: GPU vs naive"
    vd.assert_cols_equal(got, o.consolidate(sch, u), f"{what}: GPU vs oracle")
    return got


def grouped(lens, sums, rng, kw=1, vb=8, shuffle=True):
    """One group per entry of `lens`: group j is lens[j] equal rows (key j
    in every key word, val bytes and time derived from j) whose diffs are
    random but add up to sums[j] (mod 2^64)."""
    lens = np.asarray(lens, np.int64)
    n = int(lens.sum())
    gid = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    keys = np.repeat(gid[:, None], kw, axis=1) - 3   # some negative keys
    vals = ((gid[:, None] * 31 + np.arange(vb)[None, :]) % 251).astype(np.uint8)
    times = (gid % 5).astype(np.uint64)
    diffs = rng.integers(-2**62, 2**62, n).astype(np.int64)
    ends = np.cumsum(lens) - 1
    starts = ends - lens + 1
    tot = np.add.reduceat(diffs.view(np.uint64), starts)  # wraps
    want = np.asarray(sums, np.int64).view(np.uint64)
    diffs.view(np.uint64)[ends] += want - tot
    batch = [np.ascontiguousarray(keys), vals, times, diffs]
    if shuffle:
        p = rng.permutation(n)
        batch = [np.ascontiguousarray(c[p]) for c in batch]
    return tuple(batch)


def test_one_row(g, o):
    b = grouped([1], [7], np.random.default_rng(0))
    got = check(g, o, 1, 8, b, "n=1")
    assert len(got[2]) == 1


def test_two_rows_cancel(g, o):
    b = grouped([2], [0], np.random.default_rng(1))
    b[3][:] = [1, -1]
    got = check(g, o, 1, 8, b, "+1/-1")
    assert len(got[2]) == 0


@pytest.mark.parametrize("total", [5000, 0])
def test_one_group_spans_many_blocks(g, o, total):
    """5000 identical rows: one head flag, and the group's sum is carried
    across ~20 blocks and several scan tiles."""
    b = grouped([5000], [total], np.random.default_rng(2))
    got = check(g, o, 1, 8, b, f"5000 rows sum {total}")
    assert [int(d) for d in got[3]] == ([total] if total else [])


def cycle_lens(ngroups):
    return [(1, 2, 255, 256, 257)[j % 5] for j in range(ngroups)]


def test_groups_around_block_boundaries(g, o):
    """Lengths cycle 1, 2, 255, 256, 257: the running offset moves by
    771 = 3 * 256 + 3 per cycle, so over 90 cycles group starts and ends
    each fall on the last thread of a block, the first and the second.
    Every fourth group sums to zero."""
    lens = cycle_lens(450)
    sums = [0 if j % 4 == 1 else j + 1 for j in range(len(lens))]
    b = grouped(lens, sums, np.random.default_rng(3))
    starts = np.cumsum([0] + lens[:-1])
    ends = starts + np.array(lens) - 1
    for at in (starts, ends):
        assert {0, 1, 255} <= set((at % 256).tolist())
    got = check(g, o, 1, 8, b, "cycle")
    assert [int(d) for d in got[3]] == [s for s in sums if s]


@pytest.mark.parametrize("first,last", [(0, 5), (5, 0), (0, 0)])
def test_zero_sum_at_the_ends(g, o, first, last):
    lens = [3, 300, 1, 257, 2]
    sums = [first, 1, 2, 3, last]
    b = grouped(lens, sums, np.random.default_rng(4))
    got = check(g, o, 1, 8, b, f"ends {first},{last}")
    assert [int(d) for d in got[3]] == [s for s in sums if s]


def test_sum_wraps_past_2_63(g, o):
    """Three rows of 2^62 + 2^62 + 2^62 wrap to -2^62; 2^63 - 1 plus 1 wraps
    to INT64_MIN; and two INT64_MIN rows wrap to zero and vanish."""
    rng = np.random.default_rng(5)
    b = grouped([3, 2, 2, 300], [0, 0, 0, 9], rng, shuffle=False)
    b[3][:3] = 2**62
    b[3][3:5] = [2**63 - 1, 1]
    b[3][5:7] = -2**63
    p = rng.permutation(len(b[2]))
    b = tuple(np.ascontiguousarray(c[p]) for c in b)
    got = check(g, o, 1, 8, b, "wrap")
    assert [int(d) for d in got[3]] == [-2**62, -2**63, 9]


@pytest.mark.parametrize("vb", [0, 5, 8, 12])
@pytest.mark.parametrize("kw", [1, 2, 3])
def test_row_shapes(g, o, kw, vb):
    lens = cycle_lens(11) + [1] * 40
    sums = [(j % 3) - 1 for j in range(len(lens))]
    b = grouped(lens, sums, np.random.default_rng(10 * kw + vb), kw, vb)
    check(g, o, kw, vb, b, f"kw={kw} vb={vb}")


def test_past_the_grid_cap(g, o):
    """2048 * 256 + 1 rows: one more than a full grid of 256-thread blocks
    covers, so every grid-stride loop runs a second iteration. Groups of 1
    to 4 rows; the reference is the oracle and the known sums."""
    n = GRID_CAP_ROWS + 1
    rng = np.random.default_rng(6)
    lens = []
    left = n
    while left:
        step = min(left, 1 + len(lens) % 4)
        lens.append(step)
        left -= step
    sums = (np.arange(len(lens)) % 3).astype(np.int64)  # every third: zero
    b = grouped(lens, sums, rng)
    assert len(b[2]) == n
    got = check(g, o, 1, 8, b, "grid cap", naive=False)
    np.testing.assert_array_equal(np.asarray(got[3]).view(np.int64),
                                  sums[sums != 0])
