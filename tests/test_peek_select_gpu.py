"""Peek select (mz_gpu_peek_select: key range + ORDER BY / LIMIT / OFFSET
finishing) on the GPU.

Reference: a naive Python model (select_ref below). Every update ever
inserted with time <= as_of and a key inside the range goes through
test_peek_scan_gpu.scan_ref (closure in Python, wrapping sums, canonical
order); the finishing sorts those rows with a Python key that implements
include/mz_gpu.h's column comparison (stable, so ties keep the canonical
order), walks the expanded positions and keeps [offset, offset + limit).
All four output columns and the error stream are compared byte for byte;
there are no tolerances.

Garbage datum bytes under a set null byte: neither producer can make them
(mz_gpu_mfp's OUT stores zero datum bytes under a NULL, a reduce slot's
value is zero when its null byte is set), so test_nulls_garbage_datum
inserts such rows into an arrangement directly.
"""
from collections import Counter

import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd.tpch import TpchGen
from materialize_amd.workloads import Q3Dataflow, q3_top10
from test_peek_scan_gpu import (CLOSURES, MFP_DIV, _rows, build, fn_div,
                                same, scan_ref, val_words)

pytestmark = pytest.mark.gpu

KEY, VL = abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_LOOKUP
NO_NULL = abi.MZ_GPU_NO_NULL
I64_MIN, I64_MAX = -2**63, 2**63 - 1
OB = abi.order_by


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


# ------------------------------------------------------------ reference

class TotalOverflow(Exception):
    pass


def in_range(k, rng):
    """rng: None or (lo, hi, lo_inclusive, hi_inclusive), bounds key tuples
    or None."""
    if rng is None:
        return True
    lo, hi, li, hi_incl = rng
    if lo is not None and (k < lo or (k == lo and not li)):
        return False
    if hi is not None and (k > hi or (k == hi and not hi_incl)):
        return False
    return True


def abi_range(rng, kw):
    if rng is None:
        return None
    lo, hi, li, hi_incl = rng
    return abi.key_range(lo, hi, li, hi_incl, kw=kw)


def col_key(oc, k, v):
    """One order column of row (k, v) as a Python sort key: NULLs on the
    side nulls_last says, whatever desc; datums as signed ints, negated
    under desc; a NULL's datum bytes do not take part."""
    if oc.null_off != NO_NULL and v[oc.null_off] != 0:
        return (1 if oc.nulls_last else -1, 0)
    if oc.src == KEY:
        x = k[oc.off // 8]
    else:
        x = int.from_bytes(v[oc.off:oc.off + oc.width], "little", signed=True)
    return (0, -x if oc.desc else x)


def finish_ref(rows, fin):
    """rows: consolidated (key tuple, val bytes, count > 0) in canonical
    order."""
    total = sum(d for _, _, d in rows)
    if total > I64_MAX:
        raise TotalOverflow
    cols = [fin.order[j] for j in range(fin.n_order)]
    rows = sorted(rows, key=lambda r: tuple(col_key(oc, r[0], r[1])
                                            for oc in cols))
    end = None if fin.limit < 0 else fin.offset + fin.limit
    out, pos = [], 0
    for k, v, d in rows:
        lo, hi = pos, pos + d
        pos = hi
        kept = (hi if end is None else min(hi, end)) - max(lo, fin.offset)
        if kept > 0:
            out.append((k, v, kept))
    if total <= 5000:  # the same by expanding, slicing and re-grouping
        flat = [i for i, r in enumerate(rows) for _ in range(r[2])]
        regroup = [(rows[i][0], rows[i][1], c) for i, c in
                   sorted(Counter(flat[fin.offset:end]).items())]
        assert regroup == out
    return out


def rows_of(cols, kw, vb):
    keys, vals, _, diffs = cols
    keys = np.asarray(keys, np.int64).reshape(-1, kw)
    vals = np.asarray(vals, np.uint8).reshape(len(diffs), vb)
    return [(tuple(int(x) for x in keys[i]), vals[i].tobytes(),
             int(diffs[i])) for i in range(len(diffs))]


def cols_of(rows, as_of):
    return (np.array([x for r in rows for x in r[0]], np.int64),
            np.frombuffer(b"".join(r[1] for r in rows), np.uint8),
            np.full(len(rows), as_of, np.uint64),
            np.array([r[2] for r in rows], np.int64))


def select_ref(batches, as_of, rng=None, fn=None, fin=None, okw=1, ovb=0):
    """-> ((keys, vals, times, diffs), error sum, rows before finishing)."""
    kept = []
    for keys, vals, times, diffs in batches:
        m = np.array([in_range(tuple(int(x) for x in k), rng) for k in keys],
                     bool)
        kept.append((keys[m], vals[m], times[m], diffs[m]))
    cols, err = scan_ref(kept, as_of, fn)
    matched = len(cols[3])
    if fin is not None:
        cols = cols_of(finish_ref(rows_of(cols, okw, ovb), fin), as_of)
    return cols, err, matched


def check_errs(g, err, as_of, what):
    ecodes, etimes, ediffs = g.last_errs
    if err == 0:
        assert len(ecodes) == 0, f"{what}: unexpected error rows"
    else:  # one consolidated (code, as_of, sum) row
        assert ecodes.tolist() == [abi.MZ_ERR_DIVISION_BY_ZERO], what
        assert etimes.tolist() == [as_of] and ediffs.tolist() == [err], what


class Arr:
    """An arrangement with everything the model needs."""

    def __init__(self, g, kw, vb, batches, bounds):
        self.kw, self.vb, self.batches = kw, vb, batches
        self.arr = build(g, kw, vb, batches, bounds)
        self.last = max(hi for _, hi in bounds) - 1


def check(g, a, as_of, rng=None, mfp=None, fn=None, fin=None, what="",
          okw=None, ovb=None):
    okw = a.kw if okw is None else okw
    ovb = a.vb if ovb is None else ovb
    want, err, matched = select_ref(a.batches, as_of, rng, fn, fin, okw, ovb)
    got = g.peek_select(a.arr, as_of, abi_range(rng, a.kw), mfp, fin)
    what = f"{what} as_of={as_of} range={rng}"
    same(got, want, what)
    check_errs(g, err, as_of, what)
    assert g.last_peek_stats[1] == matched, f"{what}: rows_matched"
    return got


# ------------------------------------------------------------------ data

KEYS1 = [(I64_MIN,), (-7,), (-3,), (-1,), (0,), (1,), (2,), (5,), (9,),
         (I64_MAX,)]
KEYS2 = [(-1, 5), (0, I64_MIN), (0, -1), (0, 0), (0, 3), (0, I64_MAX),
         (1, -4), (1, 0), (1, 7), (2, 2)]


def gen_batches(seed, keys, vpool, inserts, rows, times_per=2):
    """`inserts` batches of `rows` updates over (keys x vpool), batch b at
    times [times_per * b, times_per * (b + 1)). Diffs are +1..+3, or -1 of a
    copy that EARLIER batches left, so net counts stay >= 0 at every time."""
    rng = np.random.default_rng(seed)
    keys = np.array(keys, np.int64)
    live, batches, bounds = {}, [], []
    for b in range(inserts):
        avail = [r for r, c in sorted(live.items()) for _ in range(c)]
        avail = [avail[i] for i in rng.permutation(len(avail))]
        ki, vi, ts, ds = [], [], [], []
        for _ in range(rows):
            if avail and rng.random() < 0.3:
                (k, v), d = avail.pop(), -1
            else:
                k, v = int(rng.integers(len(keys))), int(rng.integers(
                    len(vpool)))
                d = int(rng.integers(1, 4))
            ki.append(k)
            vi.append(v)
            ds.append(d)
            ts.append(times_per * b + int(rng.integers(times_per)))
        for k, v, d in zip(ki, vi, ds):
            live[(k, v)] = live.get((k, v), 0) + d
        batches.append((keys[ki], vpool[vi], np.array(ts, np.uint64),
                        np.array(ds, np.int64)))
        bounds.append((times_per * b, times_per * (b + 1)))
    return batches, bounds


def byte_pool(seed, n, vb):
    return np.random.default_rng(seed).integers(0, 256, (n, vb)) \
        .astype(np.uint8)


def xyz_pool():
    """20-byte vals [x i32 @0][y i64 @4][z i64 @12]: (y, z) read as one
    16-byte integer has low word y (compared unsigned) and high word z."""
    xs = [-2**31, -5, 0, 7, 2**31 - 1]
    ys = [I64_MIN, -1, 0, 1, I64_MAX]
    zs = [-1, 0, 0, 1]
    rng = np.random.default_rng(99)
    out = np.zeros((24, 20), np.uint8)
    for i in range(24):
        out[i, 0:4] = np.frombuffer(
            int(rng.choice(xs)).to_bytes(4, "little", signed=True), np.uint8)
        out[i, 4:12] = np.frombuffer(
            int(ys[rng.integers(5)]).to_bytes(8, "little", signed=True),
            np.uint8)
        out[i, 12:20] = np.frombuffer(
            int(zs[rng.integers(4)]).to_bytes(8, "little", signed=True),
            np.uint8)
    return out


def ab_pool():
    """16-byte vals [a i64][b i64] for test_peek_scan_gpu's closures: a in
    -5..5, b in 0..7 (b == 0 divides by zero under MFP_DIV)."""
    rng = np.random.default_rng(7)
    return np.stack([rng.integers(-5, 6, 24), rng.integers(0, 8, 24)], 1) \
        .astype(np.int64).view(np.uint8).reshape(24, 16)


SHAPES = {
    # name: (kw, vb, keys, val pool, inserts, rows per insert)
    "kw1-vb0-3": (1, 0, KEYS1, byte_pool(1, 1, 0), 3, 40),
    "kw1-vb16-14": (1, 16, KEYS1, ab_pool(), 14, 20),
    "kw2-vb20-3": (2, 20, KEYS2, xyz_pool(), 3, 90),
    "kw2-vb16-14": (2, 16, KEYS2, ab_pool(), 14, 20),
    "kw1-vb20-3": (1, 20, KEYS1, xyz_pool(), 3, 90),
}


@pytest.fixture(scope="module")
def arrs(g):
    out = {}
    for i, (name, (kw, vb, keys, pool, ins, rows)) in enumerate(
            SHAPES.items()):
        batches, bounds = gen_batches(500 + i, keys, pool, ins, rows)
        out[name] = Arr(g, kw, vb, batches, bounds)
        for as_of in (out[name].last // 2, out[name].last):
            d = scan_ref(batches, as_of)[0][3]
            assert len(d) and (d > 0).all(), "test data: net counts"
    return out


# --------------------------------------------------------------- identity

@pytest.mark.parametrize("name", list(SHAPES))
def test_identity_equals_peek_scan(g, arrs, name):
    """No range and no finishing: the out-batch of mz_gpu_peek_scan, byte
    for byte, and so is a finishing that is the identity."""
    a = arrs[name]
    for as_of in (0, a.last // 2, a.last):
        want = g.peek_scan(a.arr, as_of)
        for fin in (None, abi.finishing()):
            got = g.peek_select(a.arr, as_of, finishing=fin)
            same(got, want, f"{name} as_of={as_of}")
            assert len(g.last_errs[0]) == 0
        check(g, a, as_of, what=name)
        assert g.last_peek_stats[0] >= g.last_peek_stats[1] > 0


@pytest.mark.parametrize("name", ["kw1-vb16-14", "kw2-vb16-14"])
def test_identity_with_closures_and_errors(g, arrs, name):
    a = arrs[name]
    # test_peek_scan_gpu's closures carry one key word
    mfps = [m for m, _ in CLOSURES.values()] + [MFP_DIV] if a.kw == 1 \
        else [div2()[0]]
    for mfp in mfps:
        for as_of in (a.last // 2, a.last):
            want = g.peek_scan(a.arr, as_of, mfp)
            werrs = [x.tolist() for x in g.last_errs]
            got = g.peek_select(a.arr, as_of, mfp=mfp)
            same(got, want, f"{name} mfp as_of={as_of}")
            assert [x.tolist() for x in g.last_errs] == werrs
    if a.kw == 1:
        check(g, a, a.last, mfp=MFP_DIV, fn=fn_div, ovb=16, what="div")
        assert len(g.last_errs[0]) == 1


def div2():
    """MFP_DIV for two key words: (b, a / b), b == 0 errors."""
    F = abi.field
    mfp = abi.closure(
        [], [F(KEY, 0, 16)],
        [F(VL, 8, 8), F(abi.MZ_SRC_COMPUTE, abi.MZ_COMPUTE_DIV_I64, 8,
                        arg0=0, arg1=8, arg0_src=VL, arg1_src=VL)],
        abi.schema(2, 16))
    return mfp, fn_div


# ----------------------------------------------------------------- ranges

def ranges_for(keys):
    """Range cases over a sorted key pool of 10 keys (tuples)."""
    k = sorted(keys)
    lo_key, hi_key = k[2], k[7]
    w = len(k[0])
    mn, mx = (I64_MIN,) * w, (I64_MAX,) * w

    def between(a, b):  # a key tuple that is not in the pool, if any
        c = a[:-1] + (a[-1] + 1,)
        return c if a < c < b and c not in k else None

    out = [None, (None, None, True, True),              # whole
           (k[4], k[4], True, True),                    # a single key
           (k[4], k[4], True, False), (k[4], k[4], False, True),
           (hi_key, lo_key, True, True),                # lo > hi
           (k[1], k[3], True, True),                    # low (negative) keys
           (mn, mx, True, True), (mn, mx, False, False),
           (mn, None, False, True), (None, mx, True, False),
           (mn, mn, True, True), (mx, mx, True, True)]
    for li in (True, False):
        for hi_incl in (True, False):
            out.append((lo_key, hi_key, li, hi_incl))     # keys that exist
            a, b = between(k[2], k[3]), between(k[6], k[7])
            if a and b:
                out.append((a, b, li, hi_incl))            # ... that do not
    gap = between(k[4], k[5])
    if gap:
        out.append((gap, gap, True, True))              # empty, inside
    if w == 2:  # bounds that split a first word
        out += [((0, -1), (1, 0), True, True), ((0, -1), (1, 0), False, False),
                ((0, 1), (0, 2), True, True), ((0, -2), (0, 4), False, False),
                ((0, I64_MAX), (1, I64_MIN), False, True),
                ((1, I64_MIN), None, True, True),
                (None, (0, I64_MAX), True, False)]
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_ranges(g, arrs, name):
    a = arrs[name]
    keys = KEYS1 if a.kw == 1 else KEYS2
    sizes = set()
    for rng in ranges_for(keys):
        for as_of in (a.last // 2, a.last):
            got = check(g, a, as_of, rng, what=name)
            sizes.add(len(got[3]))
    assert 0 in sizes and len(sizes) > 4  # empty, partial and whole answers


def test_range_on_a_key_in_some_batches_only(g):
    pool = byte_pool(3, 4, 8)
    batches, bounds = gen_batches(11, KEYS1, pool, 3, 30, times_per=1)
    only = np.array([[777]], np.int64)
    k, v, t, d = batches[1]
    batches[1] = (np.concatenate([k, only, only]),
                  np.concatenate([v, pool[:2]]),
                  np.concatenate([t, t[:2]]), np.concatenate([d, [2, 1]]))
    a = Arr(g, 1, 8, batches, bounds)
    assert g.arr_stats(a.arr)[0] >= 2
    for as_of in (0, 1, 2):
        got = check(g, a, as_of, ((777,), (777,), True, True), what="777")
        assert len(got[3]) == (2 if as_of >= 1 else 0)
        check(g, a, as_of, ((10,), None, True, True), what="above the pool")
        check(g, a, as_of, (None, (776,), True, True), what="below 777")


# ------------------------------------------------------------- work bound

def test_work_bound(g):
    """About 5 000 vals over six batches; a range with under 2 % of the
    keys. The scan walks at least the distinct in-range (key, val) pairs
    that have any update, and at most the inserted update rows with an
    in-range key — far fewer than the arrangement holds. Retractions sit at
    later times than what they take back, so no pair cancels away inside an
    insert."""
    rng = np.random.default_rng(2024)
    batches, bounds = [], []
    for t in range(6):
        n = 1000
        keys = rng.integers(-2500, 2500, (n, 1)).astype(np.int64)
        vals = rng.integers(0, 3, (n, 1)).astype(np.int64).view(np.uint8) \
            .reshape(n, 8)
        diffs = np.ones(n, np.int64)
        if t:  # take back a tenth of the previous batch
            pk, pv = batches[-1][0][:100], batches[-1][1][:100]
            keys, vals = np.concatenate([keys, pk]), np.concatenate([vals, pv])
            diffs = np.concatenate([diffs, -np.ones(100, np.int64)])
        batches.append((keys, vals, np.full(len(diffs), t, np.uint64), diffs))
        bounds.append((t, t + 1))
    a = Arr(g, 1, 8, batches, bounds)
    total_vals = sum(len({(int(k[0]), v.tobytes()) for k, v in zip(b[0], b[1])})
                     for b in batches)
    assert total_vals > 5000
    for lo, hi in ((-40, 20), (1003, 1063), (-2500, -2440)):
        rngk = ((lo,), (hi,), True, False)
        allk = np.unique(np.concatenate([b[0].ravel() for b in batches]))
        assert ((allk >= lo) & (allk < hi)).sum() < 0.02 * len(allk)
        pairs, upds = set(), 0
        for k, v, _, _ in batches:
            for i in np.nonzero((k[:, 0] >= lo) & (k[:, 0] < hi))[0]:
                pairs.add((int(k[i, 0]), v[i].tobytes()))
                upds += 1
        check(g, a, 5, rngk, what="work bound")
        scanned = g.last_peek_stats[0]
        assert len(pairs) <= scanned <= upds, (len(pairs), scanned, upds)
        assert scanned < total_vals // 20
    check(g, a, 3, None, what="whole, as_of in the middle")
    assert g.last_peek_stats[0] <= sum(len(b[3]) for b in batches)
    g.peek_select(a.arr, 5)
    whole = g.last_peek_stats[0]
    assert whole >= total_vals * 0.5  # merges may have joined batches


# ------------------------------------------------------- finishing: order

XYZ_COLS = {"x4": dict(off=0, width=4), "y8": dict(off=4, width=8),
            "yz16": dict(off=4, width=16), "z8": dict(off=12, width=8)}


@pytest.mark.parametrize("name", ["kw1-vb20-3", "kw2-vb20-3"])
def test_order_by_one_column(g, arrs, name):
    a = arrs[name]
    for col, kwargs in XYZ_COLS.items():
        for desc in (False, True):
            fin = abi.finishing([OB(VL, desc=desc, **kwargs)])
            got = check(g, a, a.last, fin=fin, what=f"{name} {col} {desc}")
            assert len(got[3]) > 20
    for word in range(a.kw):
        for desc in (False, True):
            fin = abi.finishing([OB(KEY, 8 * word, desc=desc)], limit=25)
            check(g, a, a.last // 2, fin=fin, what=f"{name} key word {word}")


def test_order_by_two_columns_and_ties(g, arrs):
    a = arrs["kw2-vb20-3"]
    for c0, c1 in (("z8", "x4"), ("x4", "yz16"), ("yz16", "x4")):
        for d0, d1 in ((False, True), (True, False), (True, True)):
            fin = abi.finishing([OB(VL, desc=d0, **XYZ_COLS[c0]),
                                 OB(VL, desc=d1, **XYZ_COLS[c1])], offset=2)
            check(g, a, a.last, fin=fin, what=f"{c0},{c1}")
    fin = abi.finishing([OB(KEY, 8, desc=True), OB(VL, 0, 4),
                         OB(KEY, 0, desc=True), OB(VL, 12, desc=True)],
                        limit=40, offset=5)
    check(g, a, a.last, fin=fin, what="four columns")


def test_all_equal_order_values_show_canonical_order(g):
    """Every row carries the same order value, so the finishing order is the
    canonical (key, val) order — under ASC and under DESC alike."""
    rng = np.random.default_rng(8)
    n = 120
    vals = np.zeros((n, 16), np.uint8)
    vals[:, :8] = np.full(n, 42, np.int64).reshape(-1, 1).view(np.uint8) \
        .reshape(n, 8)
    vals[:, 8:] = rng.integers(0, 256, (n, 8))
    batch = (rng.integers(-9, 9, (n, 1)).astype(np.int64), vals,
             np.zeros(n, np.uint64), rng.integers(1, 3, n).astype(np.int64))
    a = Arr(g, 1, 16, [batch], [(0, 1)])
    canon = g.peek_scan(a.arr, 0)
    for desc in (False, True):
        fin = abi.finishing([OB(VL, 0, desc=desc)])
        got = check(g, a, 0, fin=fin, what="all equal")
        same(got, canon, "canonical order under ties")
        fin = abi.finishing([OB(VL, 0, desc=desc)], limit=7, offset=3)
        got = check(g, a, 0, fin=fin, what="all equal, clipped")
        assert int(got[3].sum()) == 7


# ------------------------------------------------------- finishing: NULLs

def null_cases(cols):
    """Each column description (off, width, null_off) under both directions
    and both NULL placements, and the SQL default."""
    for off, width, null_off in cols:
        for desc in (False, True):
            for nulls_last in (False, True, None):
                yield OB(VL, off, width=width, desc=desc,
                         nulls_last=nulls_last, null_off=null_off)


def test_nulls_after_the_datum_from_mfp(g):
    """Rows made by mz_gpu_mfp: [x i64 @0][null @8][y i32 @9][null @13],
    x NULL where b == 0, y NULL where a is a multiple of 3."""
    rng = np.random.default_rng(31)
    n = 200
    A = abi.x_col(abi.MZ_SRC_VAL_STREAM, 0)
    B = abi.x_col(abi.MZ_SRC_VAL_STREAM, 8)
    spec = abi.mfp_spec(abi.schema(1, 16), abi.schema(1, 14), [
        abi.x_out_key(abi.x_col(KEY, 0), 0),
        abi.x_out_val(abi.x_if(B == 0, abi.x_null("int"), A - 3), 0, 8,
                      nullable=1),
        abi.x_out_val(abi.x_if(A % 3 == 0, abi.x_null("int"), B - 2), 9, 4,
                      nullable=1)])
    batches, bounds = [], []
    for t in range(2):
        vals = np.stack([rng.integers(-6, 7, n), rng.integers(0, 4, n)], 1) \
            .astype(np.int64).view(np.uint8).reshape(n, 16)
        u = abi.make_updates(rng.integers(-4, 5, n).astype(np.int64), vals,
                             np.full(n, t, np.uint64), np.ones(n, np.int64),
                             t, t + 1)
        k, v, tm, d = g.mfp(spec, u)
        batches.append((k.reshape(-1, 1), v.reshape(-1, 14), tm, d))
        bounds.append((t, t + 1))
    a = Arr(g, 1, 14, batches, bounds)
    stored = np.concatenate([b[1] for b in batches])
    for nb in (8, 13):  # NULLs and datums on both columns
        assert 0 < int((stored[:, nb] != 0).sum()) < len(stored)
    for oc in null_cases([(0, 8, 8), (9, 4, 13)]):
        check(g, a, 1, fin=abi.finishing([oc]), what="mfp nulls")
        check(g, a, 0, fin=abi.finishing([oc], limit=9, offset=4),
              what="mfp nulls, clipped")
    fin = abi.finishing([OB(VL, 9, width=4, null_off=13, nulls_last=False),
                         OB(VL, 0, desc=True, null_off=8)])
    check(g, a, 1, fin=fin, what="two nullable columns")


def test_nulls_before_the_datum_from_reduce(g):
    """Rows made by a reduce: one 24-byte SUM slot, null byte at 0, the
    i128 at [8, 24). Keys 0..5 only ever see NULL inputs (an all-NULL SUM);
    the corrections of two pushes are the index's updates."""
    rng = np.random.default_rng(32)
    aggs = [abi.Aggregate(func=abi.MZ_AGG_SUM_I64, off=0, width=8,
                          is_float=0, nullable=1)]
    op = g.reduce_create(abi.reduce_spec(aggs, abi.schema(1, 16)))
    batches, bounds = [], []
    try:
        for t in range(2):
            n = 150
            keys = rng.integers(0, 40, n).astype(np.int64)
            keys[:6] = np.arange(6)
            vals = np.zeros((n, 16), np.uint8)
            vals[:, :8] = (rng.integers(-2**40, 2**40, n) * 2**22) \
                .astype(np.int64).reshape(-1, 1).view(np.uint8).reshape(n, 8)
            vals[:, 8] = (keys < 6) | (rng.random(n) < 0.2)
            u = abi.make_updates(keys, vals, np.full(n, t, np.uint64),
                                 rng.integers(1, 2000, n).astype(np.int64),
                                 t, t + 1)
            k, v, tm, d = g.reduce_push(op, u)
            batches.append((k.reshape(-1, 1), v.reshape(-1, 24), tm, d))
            bounds.append((t, t + 1))
    finally:
        g.reduce_drop(op)
    assert (batches[1][3] < 0).any()  # the second push retracts old sums
    a = Arr(g, 1, 24, batches, bounds)
    for as_of in (0, 1):
        view = rows_of(g.peek_scan(a.arr, as_of), 1, 24)
        nulls = [r for r in view if r[1][0] != 0]
        assert len(nulls) >= 6 and len(nulls) < len(view)
        # sums beyond an i64: the high word takes part in the order
        assert any(r[1][16:24] not in (b"\0" * 8, b"\xff" * 8) for r in view)
        for oc in null_cases([(8, 16, 0)]):
            check(g, a, as_of, fin=abi.finishing([oc]), what="reduce slot")
            check(g, a, as_of, fin=abi.finishing([oc, OB(KEY, 0, desc=True)],
                                                 limit=10),
                  what="reduce slot top 10")


def test_nulls_garbage_datum(g):
    """Rows stored directly with random datum bytes under a set null byte:
    NULLs are equal to each other, so they appear in canonical order."""
    rng = np.random.default_rng(33)
    n = 100
    vals = rng.integers(0, 256, (n, 9)).astype(np.uint8)
    vals[:, 8] = rng.integers(0, 2, n) * rng.integers(1, 256, n)
    batch = (rng.integers(-5, 5, (n, 1)).astype(np.int64), vals,
             np.zeros(n, np.uint64), np.ones(n, np.int64))
    a = Arr(g, 1, 9, [batch], [(0, 1)])
    for oc in null_cases([(0, 8, 8), (0, 4, 8), (4, 4, 8)]):
        got = check(g, a, 0, fin=abi.finishing([oc]), what="garbage")
        rows = rows_of(got, 1, 9)
        nulls = [(r[0], val_words(r[1])) for r in rows if r[1][8]]
        assert len(nulls) > 20 and nulls == sorted(nulls)
        first_null = next(i for i, r in enumerate(rows) if r[1][8])
        assert first_null == (len(rows) - len(nulls) if oc.nulls_last else 0)


# ----------------------------------------------- finishing: multiplicities

def test_offsets_and_limits_across_counts(g):
    """Counts 3, 1, 4, 2, 5 in order: every offset from 0 to beyond the
    total with every limit, so windows start and end inside a row's copies,
    at its edges, at the total and past it."""
    batch = _rows([(k, 100 - k, 0, c)
                   for k, c in enumerate([3, 1, 4, 2, 5])])
    a = Arr(g, 1, 8, [batch], [(0, 1)])
    order = [OB(VL, 0)]  # descending key order
    for offset in range(0, 18):
        for limit in (None, 0, 1, 2, 3, 6, 14, 15, 16, I64_MAX):
            fin = abi.finishing(order, limit=limit, offset=offset)
            got = check(g, a, 0, fin=fin, what=f"off={offset} lim={limit}")
            total = max(0, 15 - offset)
            assert int(got[3].sum()) == \
                (total if limit is None else min(total, limit))
    fin = abi.finishing(order, limit=None, offset=2**64 - 1)
    assert len(check(g, a, 0, fin=fin, what="huge offset")[3]) == 0
    fin = abi.finishing(order, limit=I64_MAX, offset=2**64 - 2)
    assert len(check(g, a, 0, fin=fin, what="offset + limit wraps")[3]) == 0


def test_projection_collapses_before_finishing(g, arrs):
    """The mfp drops a: rows that differ only in a add their counts, and the
    finishing sees the sums."""
    a = arrs["kw1-vb16-14"]
    mfp, fn = CLOSURES["project"]
    plain = g.peek_select(a.arr, a.last)
    for fin in (abi.finishing([OB(VL, 0, desc=True)], limit=11, offset=3),
                abi.finishing([OB(VL, 0), OB(KEY, 0, desc=True)], limit=30),
                abi.finishing(offset=17)):
        got = check(g, a, a.last, mfp=mfp, fn=fn, fin=fin, ovb=8,
                    what="project")
        assert g.last_peek_stats[1] < len(plain[3])
        assert len(got[3]) > 0
    mfp, fn = CLOSURES["mul"]
    fin = abi.finishing([OB(VL, 8, desc=True), OB(VL, 0)], limit=20)
    check(g, a, a.last // 2, ((-3,), (5,), True, False), mfp, fn, fin,
          what="computed column, range")


def test_huge_counts(g):
    big = 2**62
    batch = _rows([(1, 10, 0, big), (2, 20, 0, big - 1), (3, 30, 1, big)])
    a = Arr(g, 1, 8, [batch], [(0, 2)])
    # as of 0: total 2^63 - 1, the largest accepted
    for fin in (abi.finishing(),
                abi.finishing([OB(KEY, 0, desc=True)]),
                abi.finishing([OB(KEY, 0, desc=True)], offset=big - 2,
                              limit=3),
                abi.finishing([OB(VL, 0)], offset=5, limit=big),
                abi.finishing(offset=I64_MAX - 1),
                abi.finishing(offset=I64_MAX)):
        check(g, a, 0, fin=fin, what="2^62 + (2^62 - 1)")
    got = g.peek_select(a.arr, 0, finishing=abi.finishing(
        [OB(KEY, 0, desc=True)], offset=big - 2, limit=3))
    assert got[0].tolist() == [2, 1] and got[3].tolist() == [1, 2]
    # as of 1: three rows of about 2^62 exceed an i64
    from materialize_amd._ffi import MzGpuError
    with pytest.raises(TotalOverflow):
        select_ref(a.batches, 1, fin=abi.finishing(), okw=1, ovb=8)
    for fin in (abi.finishing(), abi.finishing(limit=1),
                abi.finishing([OB(KEY, 0)], limit=1)):
        with pytest.raises(MzGpuError, match="peek_select: total "
                                             "multiplicity exceeds int64"):
            g.peek_select(a.arr, 1, finishing=fin)
    check(g, a, 1, what="no finishing, no total")  # context still usable
    exact = _rows([(1, 10, 0, big), (2, 20, 0, big), (3, 30, 0, big)])
    b = Arr(g, 1, 8, [exact], [(0, 1)])
    with pytest.raises(MzGpuError, match="total multiplicity exceeds int64"):
        g.peek_select(b.arr, 0, finishing=abi.finishing(limit=10))


# ------------------------------------- range and finishing together, errors

def test_range_finishing_and_error_rows(g, arrs):
    a = arrs["kw1-vb16-14"]
    fin = abi.finishing([OB(VL, 8, desc=True), OB(VL, 0)], limit=12,
                        offset=1)
    seen = 0
    for rng in (None, ((-3,), (5,), True, True), ((0,), None, False, True),
                ((100,), None, True, True)):
        for as_of in (a.last // 2, a.last):
            check(g, a, as_of, rng, MFP_DIV, fn_div, fin, what="div")
            seen += len(g.last_errs[0])
            # the error stream is the unfinished peek's
            errs = [x.tolist() for x in g.last_errs]
            g.peek_select(a.arr, as_of, abi_range(rng, 1), MFP_DIV)
            assert [x.tolist() for x in g.last_errs] == errs
    assert seen >= 2
    a2 = arrs["kw2-vb16-14"]
    mfp, fn = div2()
    fin = abi.finishing([OB(KEY, 8, desc=True), OB(VL, 8)], limit=9)
    check(g, a2, a2.last, ((0, -1), (1, 0), True, True), mfp, fn, fin,
          what="div, two words")


def test_refusals(g, arrs):
    from materialize_amd._ffi import MzGpuError
    batch = _rows([(1, 10, 0, 1), (2, 20, 0, -1), (3, 30, 0, 2)])
    neg = Arr(g, 1, 8, [batch], [(0, 1)])
    with pytest.raises(MzGpuError, match=r"peek_select: negative "
                                         r"multiplicity \(1 rows\)"):
        g.peek_select(neg.arr, 0, finishing=abi.finishing(limit=1))
    with pytest.raises(MzGpuError, match="peek_select: negative"):
        g.peek_select(neg.arr, 0)
    # the negative row is outside the range / allowed without a finishing
    check(g, neg, 0, ((3,), None, True, True), fin=abi.finishing(limit=1))
    got = g.peek_select(neg.arr, 0, allow_negative=True)
    same(got, g.peek_scan(neg.arr, 0, allow_negative=True), "allow_negative")
    with pytest.raises(MzGpuError, match="a finishing cannot be combined "
                                         "with allow_negative"):
        g.peek_select(neg.arr, 0, finishing=abi.finishing(),
                      allow_negative=True)
    # as_of before the compaction frontier
    a = Arr(g, 1, 8, *gen_batches(5, KEYS1, byte_pool(5, 3, 8), 3, 20, 1))
    g.arr_set_logical_compaction(a.arr, 2)
    with pytest.raises(MzGpuError, match="peek_select: as_of 1 is before "
                                         "the compaction frontier 2"):
        g.peek_select(a.arr, 1, finishing=abi.finishing(limit=3))
    check(g, a, 2, ((-3,), (5,), True, True), fin=abi.finishing(limit=3))
    # what peek_scan refuses, with this entry's prefix
    vl = g.arr_create(abi.schema(1, abi.MZ_GPU_VARLEN))
    with pytest.raises(MzGpuError, match="peek_select: varlen"):
        g.peek_select(vl, 0)
    bad = abi.closure([], [abi.field(KEY, 0, 8)],
                      [abi.field(abi.MZ_SRC_VAL_STREAM, 0, 16)],
                      abi.schema(1, 16))
    with pytest.raises(MzGpuError, match="peek_select: mfp reads "
                                         "MZ_SRC_VAL_STREAM"):
        g.peek_select(arrs["kw1-vb16-14"].arr, 0, mfp=bad)


def test_c_layer_refuses_bad_ranges_and_orders(g, arrs):
    """The rules test_peek_select_plan.py holds the Python layer to, asked
    of the C entry with hand-made structs."""
    from materialize_amd._ffi import MzGpuError
    a = arrs["kw1-vb16-14"]

    def rng(lk, lo, hk, hi):
        r = abi.KeyRange(lo_kind=lk, hi_kind=hk)
        r.lo[0], r.lo[1] = lo
        r.hi[0], r.hi[1] = hi
        return r

    def fin(*cols):
        f = abi.Finishing(n_order=len(cols), limit=-1)
        for j, c in enumerate(cols[:4]):
            f.order[j] = abi.PeekOrder(**c)
        return f

    K = dict(src=KEY, width=8, null_off=NO_NULL)
    V = dict(src=VL, width=8, null_off=NO_NULL)
    for r, msg in (
            (rng(3, (0, 0), 1, (0, 0)), "range: unknown bound kind 3"),
            (rng(1, (0, 1), 1, (0, 0)), "range: nonzero bound word beyond"),
            (rng(0, (4, 0), 1, (0, 0)),
             "range: nonzero bound word on an unbounded side")):
        with pytest.raises(MzGpuError, match="peek_select: " + msg):
            g.peek_select(a.arr, 0, key_range=r)
    f5 = fin(*[dict(K, off=0)] * 5)
    for f, msg in (
            (f5, "n_order must be at most 4"),
            (fin(dict(V, src=1, off=0)), "order column 0: src must be"),
            (fin(dict(K, off=0, width=4)), "a key column must be width 8"),
            (fin(dict(K, off=8)), "word boundary inside the out key"),
            (fin(dict(K, off=0, null_off=2)), "takes no null_off"),
            (fin(dict(K, off=0), dict(V, off=0, width=2)),
             "order column 1: width must be 4, 8 or 16"),
            (fin(dict(V, off=9)), "order column 0 reads past the out val"),
            (fin(dict(V, off=0, null_off=16)), "null_off is past"),
            (fin(dict(V, off=0, width=16, null_off=15)),
             "inside its own datum"),
            (fin(dict(V, off=0, desc=2)), "desc and nulls_last"),
            (fin(dict(V, off=0, nulls_last=7)), "desc and nulls_last")):
        with pytest.raises(MzGpuError, match=msg) as e:
            g.peek_select(a.arr, 0, finishing=f)
        assert str(e.value).startswith("peek_select: ")
    # the order columns are checked against the mfp's OUT row: 8 val bytes
    proj = CLOSURES["project"][0]
    with pytest.raises(MzGpuError, match="reads past the out val"):
        g.peek_select(a.arr, 0, mfp=proj, finishing=fin(dict(V, off=8)))
    check(g, a, a.last, fin=fin(dict(V, off=8)), what="after refusals")


# ------------------------------------------------------------------- fuzz

def test_fuzz(g, arrs):
    """100 seeded cases: a shape, an as_of, a range from the key pool (or
    beside it), one of the closures where the shape takes them, up to three
    order columns with random direction and NULL placement, and a window."""
    rng = np.random.default_rng(4242)
    names = list(SHAPES)
    kept_some = clipped = ranged = 0
    for case in range(100):
        name = names[rng.integers(len(names))]
        a = arrs[name]
        pool = sorted(KEYS1 if a.kw == 1 else KEYS2)
        as_of = int(rng.integers(0, a.last + 1))
        r = None
        if rng.random() < 0.7:
            def bound():
                if rng.random() < 0.2:
                    return None
                k = list(pool[rng.integers(len(pool))])
                if rng.random() < 0.3 and abs(k[-1]) < 2**62:
                    k[-1] += int(rng.integers(-1, 2))
                return tuple(k)
            r = (bound(), bound(), bool(rng.integers(2)),
                 bool(rng.integers(2)))
            ranged += 1
        mfp = fn = None
        okw, ovb = a.kw, a.vb
        if name == "kw1-vb16-14" and rng.random() < 0.6:
            which = ["val-filter", "key-filter", "project", "mul", "div"][
                rng.integers(5)]
            mfp, fn = (MFP_DIV, fn_div) if which == "div" else CLOSURES[which]
            ovb = mfp.out.val_bytes
        elif name == "kw2-vb16-14" and rng.random() < 0.4:
            mfp, fn = div2()
        cands = [dict(src=KEY, off=8 * w) for w in range(okw)]
        cands += [dict(src=VL, off=o, width=w)
                  for w in (4, 8, 16) for o in range(0, ovb - w + 1, 4)]
        cols = []
        for _ in range(rng.integers(0, 4)):
            c = dict(cands[rng.integers(len(cands))])
            if c["src"] == VL and rng.random() < 0.4:
                free = [b for b in range(ovb)
                        if not c["off"] <= b < c["off"] + c["width"]]
                if free:
                    c["null_off"] = free[rng.integers(len(free))]
            cols.append(OB(desc=bool(rng.integers(2)),
                           nulls_last=[None, False, True][rng.integers(3)],
                           **c))
        limit = [None, 0, 1, 7, 50][rng.integers(5)]
        offset = [0, 0, 1, 5, 60][rng.integers(5)]
        fin = abi.finishing(cols, limit=limit, offset=offset)
        got = check(g, a, as_of, r, mfp, fn, fin, what=f"fuzz {case} {name}",
                    okw=okw, ovb=ovb)
        kept_some += len(got[3]) > 0
        clipped += len(got[3]) < g.last_peek_stats[1]
    assert kept_some > 25 and clipped > 15 and ranged > 50


# --------------------------------------------------------------------- Q3

def test_q3_top10(g):
    """Q3's ORDER BY revenue DESC, o_orderdate LIMIT 10 read from the output
    index equals the model's finishing of the whole view, after load and
    after two churn steps; a key range on l_orderkey composes with it."""
    df = Q3Dataflow(g, index_output=True)
    gen = TpchGen(sf=0.01, seed=3)
    df.load(gen)
    top10 = q3_top10()
    for t in (0, 1, 2):
        if t:
            _, corr = df.step(gen.churn(2000), t)
            if corr is not None:
                corr.release()
        view = df.peek_result(t)
        rows = rows_of(view, 2, 24)
        assert len(rows) > 50
        want = cols_of(finish_ref(rows, top10), t)
        got = df.peek_result(t, finishing=top10)
        same(got, want, f"Q3 top 10 at {t}")
        assert got[3].tolist() == [1] * 10
        rev = [int.from_bytes(r[1][8:24], "little", signed=True)
               for r in rows_of(got, 2, 24)]
        assert rev == sorted(rev, reverse=True) and rev[0] == max(
            int.from_bytes(r[1][8:24], "little", signed=True) for r in rows)
        mid = sorted(r[0][0] for r in rows)[len(rows) // 2]
        kr = abi.key_range(lo=(mid, I64_MIN), kw=2)
        upper = [r for r in rows if r[0][0] >= mid]
        same(df.peek_result(t, finishing=top10, key_range=kr),
             cols_of(finish_ref(upper, top10), t), f"Q3 top 10 above {mid}")
        same(df.peek_result(t, key_range=kr), cols_of(upper, t),
             f"Q3 rows above {mid}")
