"""Temporal filter (mz_gpu_temporal_* / k_temporal_eval,
k_temporal_release) on the GPU.

Reference: the naive model below (class Model). Per input update it runs the
row semantics of include/mz_gpu.h with Python ints (filters and projection
as a Python function, the bounds in spec order, v = datum + add unbounded),
keeps every emitted (key, val, time) -> wrapping diff sum in a dict, and for
a push [lower, upper) expects exactly the entries with time < upper, zeros
dropped, in the engine's canonical order (keys as signed tuples, vals as
little-endian u64 words, then time), plus the consolidated (code, time,
diff) error rows. All four output columns are compared byte for byte, and
after every push `stats` is compared with the model's held count, smallest
held time and frontier. The CPU oracle has no temporal filter.
"""
import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

pytestmark = pytest.mark.gpu

KEY, VS, VL, CP = (abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_STREAM,
                   abi.MZ_SRC_VAL_LOOKUP, abi.MZ_SRC_COMPUTE)
LOWER, UPPER = abi.MZ_TB_LOWER, abi.MZ_TB_UPPER
GE, GT, LT, LE, EQ = (abi.MZ_CMP_GE, abi.MZ_CMP_GT, abi.MZ_CMP_LT,
                      abi.MZ_CMP_LE, abi.MZ_CMP_EQ)
NONE = 2**64 - 1
I64_MIN = -2**63
ERR_CODE = abi.MZ_ERR_TIMESTAMP_OUT_OF_RANGE


# ------------------------------------------------------------ reference

def wrap(d):
    return ((d + 2**63) % 2**64) - 2**63


def val_words(v):
    return tuple(int.from_bytes(v[o:o + 8], "little")
                 for o in range(0, len(v), 8))


def i64_at(v, off):
    return int.from_bytes(v[off:off + 8], "little", signed=True)


class Model:
    """fn(key tuple, val bytes) -> None (filtered) | (out key tuple, out val
    bytes); None = the row as it is."""

    def __init__(self, bounds, fn=None, until=None):
        self.bounds = [b for x in bounds
                       for b in (x if isinstance(x, list) else [x])]
        self.fn = fn
        self.until = NONE if until is None else until
        self.held = {}
        self.frontier = NONE

    def _row(self, key, val, t, d, errs):
        out = (key, val) if self.fn is None else self.fn(key, val)
        if out is None:
            return
        kbytes = b"".join(k.to_bytes(8, "little", signed=True) for k in key)
        lo, hi = t, None
        for b in self.bounds:
            src = kbytes if b.src == KEY else val
            if b.nullable and src[b.off + b.width] != 0:
                return
            v = int.from_bytes(src[b.off:b.off + b.width], "little",
                               signed=True) + b.add
            if v < 0:
                errs[(ERR_CODE, t)] = wrap(errs.get((ERR_CODE, t), 0) + d)
                return
            if b.kind == LOWER:
                lo = max(lo, v)
            else:
                hi = v if hi is None else min(hi, v)
        if hi is not None and hi <= lo:
            return
        for time, diff in ((lo, d), (hi, wrap(-d))):
            if time is not None and time < self.until:
                k = (out[0], out[1], time)
                self.held[k] = wrap(self.held.get(k, 0) + diff)

    def push(self, keys, vals, times, diffs, lower, upper):
        """-> ((keys, vals, times, diffs), (ecodes, etimes, ediffs))."""
        errs = {}
        for i in range(len(times)):
            self._row(tuple(int(x) for x in keys[i]), vals[i].tobytes(),
                      int(times[i]), int(diffs[i]), errs)
        rows = sorted(((k, v, t, d) for (k, v, t), d in self.held.items()
                       if t < upper and d != 0),
                      key=lambda r: (r[0], val_words(r[1]), r[2]))
        self.held = {k: d for k, d in self.held.items()
                     if k[2] >= upper and d != 0}
        self.frontier = upper
        e = sorted((c, t, d) for (c, t), d in errs.items() if d != 0)
        return ((np.array([x for r in rows for x in r[0]], np.int64),
                 np.frombuffer(b"".join(r[1] for r in rows), np.uint8),
                 np.array([r[2] for r in rows], np.uint64),
                 np.array([r[3] for r in rows], np.int64)),
                (np.array([x[0] for x in e], np.uint64),
                 np.array([x[1] for x in e], np.uint64),
                 np.array([x[2] for x in e], np.int64)))

    def stats(self):
        return (len(self.held),
                min((k[2] for k in self.held), default=NONE), self.frontier)


def same(got, want, what, cols=("keys", "vals", "times", "diffs")):
    for a, b, col in zip(got, want, cols):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype.itemsize == b.dtype.itemsize, f"{what}: {col} dtype"
        np.testing.assert_array_equal(
            np.ascontiguousarray(a).view(np.uint8),
            np.ascontiguousarray(b).view(np.uint8), err_msg=f"{what}: {col}")


class Rig:
    """One operator next to its model; every push and tick is compared."""

    def __init__(self, g, sch, bounds, mfp=None, fn=None, until=None,
                 initial_rows=0):
        self.g = g
        self.kw, self.vb = sch.key_words, sch.val_bytes
        spec = abi.temporal_spec(sch, bounds, mfp=mfp, until=until,
                                 initial_rows=initial_rows)
        self.op = g.temporal_create(spec)
        self.model = Model(bounds, fn, until)
        assert g.temporal_stats(self.op) == (0, NONE, NONE)

    def updates(self, keys, vals, times, diffs, lower, upper):
        return abi.make_updates(
            np.ascontiguousarray(keys, np.int64).ravel(),
            np.ascontiguousarray(vals).ravel() if self.vb else None,
            times, diffs, lower, upper)

    def push(self, keys, vals, times, diffs, lower, upper, what=""):
        n = len(times)
        keys = np.asarray(keys, np.int64).reshape(n, self.kw)
        vals = np.ascontiguousarray(vals).view(np.uint8).reshape(n, self.vb)
        times = np.asarray(times, np.uint64)
        diffs = np.asarray(diffs, np.int64)
        want, want_errs = self.model.push(keys, vals, times, diffs, lower,
                                          upper)
        got = self.g.temporal_push(
            self.op, self.updates(keys, vals, times, diffs, lower, upper))
        what = f"{what} push [{lower}, {upper})"
        same(got, want, what)
        same(self.g.last_errs, want_errs, what + " errors",
             ("codes", "times", "diffs"))
        assert self.g.temporal_stats(self.op) == self.model.stats(), what
        return got

    def tick(self, upper, what=""):
        e = np.empty(0, np.int64)
        return self.push(e, np.empty(0, np.uint8), e, e,
                         self.model.frontier, upper, what + " tick")

    def drop(self):
        self.g.temporal_drop(self.op)


def ab_vals(a, b):
    """16-byte vals [a i64][b i64]."""
    return np.stack([np.asarray(a), np.asarray(b)], 1).astype(np.int64) \
        .view(np.uint8).reshape(len(a), 16)


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


SCH = abi.schema(1, 16)
# mz_now() >= a AND mz_now() < b over vals [a][b]
AB = [abi.time_bound(GE, VS, 0), abi.time_bound(LT, VS, 8)]


# ------------------------------------------- wave edges, exact prefixes

# (a, b) per row class for a push [10, 20) at t = 10 with until = 28:
CLASSES = [(0, 5),     # hi <= lo: nothing
           (0, 15),    # +d at 10 and -d at 15: two ready
           (0, 25),    # one ready, one held
           (22, 27),   # two held
           (-5, 15),   # a < 0: one error row
           (12, 20),   # ready at 12; hi == upper stays held
           (22, 30),   # hi >= until: one held only
           (0, 29)]    # hi >= until: one ready only


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_wave_edges(g, n):
    """The row index decides what a row emits (0, 1 or 2 ready/held rows, 0
    or 1 error rows), so a miscounted wave prefix shifts every later row.
    4099 spans several blocks and a partial last wave."""
    i = np.arange(n)
    # rotate so that every size meets several classes
    cls = [CLASSES[(j + n) % len(CLASSES)] for j in i]
    r = Rig(g, SCH, AB, until=28)
    r.push(i % 50 - 25, ab_vals([c[0] for c in cls], [c[1] for c in cls]),
           np.full(n, 10), 1 + i % 3, 10, 20, f"n={n}")
    r.tick(40, f"n={n}")
    assert r.model.stats()[0] == 0
    r.drop()


# ------------------------------------------------------------ comparators

@pytest.mark.parametrize("cmp", [GE, GT, LT, LE, EQ],
                         ids=["ge", "gt", "lt", "le", "eq"])
@pytest.mark.parametrize("src, off, width", [(KEY, 0, 8), (KEY, 0, 4),
                                             (VS, 8, 8), (VS, 4, 4)],
                         ids=["key8", "key4", "val8", "val4"])
def test_comparators(g, cmp, src, off, width):
    """`mz_now() <cmp> datum + 3` through abi.time_bound, datums on both
    sides of the input time 20 and of the upper 24. >= and > leave rows
    without an upper bound (only +d); < and <= keep lo = t."""
    n = 40
    datum = np.arange(n) + 1  # + 3: 4 .. 43
    vals = np.zeros((n, 4), np.int32)
    vals[:, 1] = datum        # the 4-byte datum at 4
    vals[:, 2] = datum        # the low half of the 8-byte datum at 8
    r = Rig(g, SCH, abi.time_bound(cmp, src, off, width=width, add=3))
    r.push(datum, vals.view(np.uint8), np.full(n, 20), np.full(n, 2), 20,
           24, "cmp")
    r.tick(30, "cmp")
    r.tick(100, "cmp")
    r.drop()


def test_bounds_combine(g):
    """Two lower bounds take the max and two upper bounds the min; a lower
    bound in the past leaves the output time at t; an empty window (hi < lo
    and hi == lo) yields nothing."""
    bounds = [abi.time_bound(GE, VS, 0), abi.time_bound(GE, KEY, 0, add=2),
              abi.time_bound(LT, VS, 8), abi.time_bound(LE, KEY, 0, add=9)]
    #        key  a   b      lowers (a, key+2), uppers (b, key+10), t = 10
    rows = [(5, 11, 14),   # lo 11, hi min(14, 15) = 14
            (9, 3, 30),    # lo max(3, 11) = 11, hi min(30, 19) = 19
            (10, 12, 12),  # lo 12 == hi 12: nothing
            (0, 13, 40),   # hi 10 < lo 13: nothing
            (8, 12, 12),   # lo 12, hi 12: nothing
            (3, 0, 11),    # lowers in the past: lo = t = 10; hi 11
            (20, 0, 50)]   # lo 22 (held), hi 30
    r = Rig(g, SCH, bounds)
    r.push([x[0] for x in rows],
           ab_vals([x[1] for x in rows], [x[2] for x in rows]),
           np.full(len(rows), 10), np.arange(len(rows)) + 1, 10, 12,
           "combine")
    assert r.model.stats()[0] == 4  # 14, 19, 22, 30
    r.tick(23, "combine")
    r.tick(31, "combine")
    assert r.model.stats() == (0, NONE, 31)
    r.drop()


def test_no_upper_bound_emits_only_plus(g):
    r = Rig(g, SCH, [abi.time_bound(GE, VS, 0)])
    got = r.push([1, 2, 3], ab_vals([0, 7, 9], [0, 0, 0]), [5, 5, 5],
                 [1, 1, 1], 5, 8, "lower only")
    assert got[3].tolist() == [1, 1] and got[2].tolist() == [5, 7]
    got = r.tick(50, "lower only")
    assert got[3].tolist() == [1] and r.model.stats() == (0, NONE, 50)
    r.drop()


# ------------------------------------------------- the boundary of release

def test_release_boundary(g):
    """hi == upper stays held, hi == upper - 1 is released in this push; the
    tick to upper + 1 releases the first."""
    r = Rig(g, SCH, AB)
    got = r.push([1, 2], ab_vals([0, 0], [20, 19]), [10, 10], [1, 1], 10,
                 20, "boundary")
    assert got[2].tolist() == [10, 10, 19]
    assert r.model.stats() == (1, 20, 20)
    got = r.tick(21, "boundary")
    assert (got[0].tolist(), got[2].tolist(), got[3].tolist()) == \
        ([1], [20], [-1])
    assert r.model.stats() == (0, NONE, 21)
    r.drop()


def test_cancellation(g):
    """Insert n rows at t, delete them at t + 1, window far in the future:
    the held -d of the insert cancels the +d of the deletion."""
    n = 300
    i = np.arange(n)
    vals = ab_vals(np.zeros(n), 10**6 + i % 7)
    r = Rig(g, SCH, AB)
    r.push(i % 40, vals, np.full(n, 3), np.ones(n), 3, 4, "insert")
    assert 0 < r.model.stats()[0] <= n
    r.push(i % 40, vals, np.full(n, 4), -np.ones(n), 4, 5, "delete")
    assert r.model.stats() == (0, NONE, 5)
    for upper in (6, 10**6 + 3, 10**6 + 100):
        assert len(r.tick(upper, "after")[2]) == 0
    r.drop()


def test_multi_timestamp_delta_and_ticks(g):
    """One delta with three distinct times; a tick across several windows'
    ends, a tick across none (the skipped release pass leaves state and
    stats exact), a delta pushed while the pass is skipped."""
    n = 90
    i = np.arange(n)
    t = 10 + i % 3
    r = Rig(g, SCH, AB)
    r.push(i % 11,
           ab_vals(np.minimum(t - 1 + i % 4, 12), 20 + 5 * (i % 6)), t,
           1 + i % 2, 10, 13, "three times")
    held0 = r.model.stats()
    assert held0[1] == 20
    assert len(r.tick(15, "across none")[2]) == 0
    assert r.model.stats() == (held0[0], 20, 15)
    assert len(r.tick(15, "empty tick")[2]) == 0
    # new rows while nothing is due: appended behind the resident rows
    r.push([3, 4], ab_vals([0, 0], [25, 70]), [16, 17], [5, 5], 15, 18,
           "skip + new")
    got = r.tick(36, "across several")  # 20, 25, 30, 35
    assert sorted(set(got[2].tolist())) == [20, 25, 30, 35]
    r.tick(100, "rest")
    assert r.model.stats() == (0, NONE, 100)
    r.drop()


# ----------------------------------------- NULL and out-of-range bounds

def test_null_and_out_of_range_bounds(g):
    """A nullable bound with the indicator set drops the row; datum + add <
    0 gives the error row at (t, d) and no ok row; the error stream
    consolidates to one row per (code, time)."""
    sch = abi.schema(1, 24)  # [a i64][null byte of a, pad][b i64]
    bounds = [abi.time_bound(GE, VS, 0, add=-4, nullable=1),
              abi.time_bound(LT, VS, 16)]
    n = 200
    i = np.arange(n)
    a = np.where(i % 5 == 0, 2, 14 + i % 3)  # 2 - 4 < 0: error
    vals = np.zeros((n, 3), np.int64)
    vals[:, 0] = a
    vals[:, 1] = (i % 7 == 0)                # NULL a (wins over the error)
    vals[:, 2] = np.where(i % 9 == 0, -1, 30)  # b < 0: error
    t = 10 + i % 2
    r = Rig(g, sch, bounds)
    r.push(i % 13, vals.view(np.uint8), t, 1 + i % 4, 10, 12, "null/oor")
    ecodes, etimes, ediffs = g.last_errs
    assert ecodes.tolist() == [ERR_CODE, ERR_CODE]
    assert etimes.tolist() == [10, 11]
    r.tick(40, "null/oor")
    assert len(g.last_errs[0]) == 0
    # errors that cancel: +d and -d at one time leave no error row
    r.push([1, 1], np.array([[2, 0, 30], [2, 0, 30]], np.int64)
           .view(np.uint8), [40, 40], [3, -3], 40, 41, "errors cancel")
    assert len(g.last_errs[0]) == 0
    r.drop()


def test_exact_bound_arithmetic(g):
    """v = datum + add is exact: INT64_MAX + INT64_MAX is a legal (far)
    bound, INT64_MIN + add < 0 an error, neither wraps."""
    big = 2**63 - 1
    r = Rig(g, SCH, [abi.time_bound(GE, VS, 0, add=big),
                     abi.time_bound(LT, VS, 8, add=big)])
    r.push([1, 2, 3], ab_vals([-big, -big, I64_MIN], [big, -big + 9, 0]),
           [5, 5, 5], [1, 1, 1], 5, 6, "exact")
    assert r.model.stats() == (2, 9, 6)  # -1 at 9 and at 2^64 - 2
    assert g.last_errs[2].tolist() == [1]
    r.tick(10, "exact")
    assert r.model.stats() == (1, 2**64 - 2, 10)
    r.drop()


# ------------------------------------------------------------------ until

def test_until(g):
    """lo >= until: nothing at all, even if hi exists; hi >= until: only the
    +d side and nothing held for it; hi == until - 1: kept."""
    rows = [(1, 50, 60),   # lo 50 == until: nothing
            (2, 55, 70),   # lo > until: nothing
            (3, 0, 50),    # hi == until: +d only
            (4, 0, 80),    # hi > until: +d only
            (5, 0, 49),    # hi == until - 1: kept, held
            (6, 49, 52)]   # lo == until - 1 held, hi dropped
    r = Rig(g, SCH, AB, until=50)
    got = r.push([x[0] for x in rows],
                 ab_vals([x[1] for x in rows], [x[2] for x in rows]),
                 np.full(len(rows), 10), np.ones(len(rows)), 10, 11, "until")
    assert got[0].tolist() == [3, 4, 5]
    assert r.model.stats() == (2, 49, 11)
    got = r.tick(60, "until")
    assert (got[0].tolist(), got[3].tolist()) == ([5, 6], [-1, 1])
    r.drop()


# --------------------------------------------------------------- wrapping

def test_wrapping_diffs(g):
    """-INT64_MIN stays INT64_MIN, and diffs that cancel only after
    wrapping do cancel, in ready and in held."""
    r = Rig(g, SCH, AB)
    vals = ab_vals([0, 0, 0], [30, 30, 30])
    got = r.push([1, 2, 2], vals, [10, 10, 10], [I64_MIN, I64_MIN, I64_MIN],
                 10, 11, "wrap")
    # key 1: I64_MIN at 10; key 2: I64_MIN + I64_MIN wraps to 0
    assert (got[0].tolist(), got[3].tolist()) == ([1], [I64_MIN])
    assert r.model.stats() == (1, 30, 11)
    got = r.tick(31, "wrap")
    assert got[3].tolist() == [I64_MIN]
    big = 2**62
    got = r.push([7] * 4, ab_vals([0] * 4, [50] * 4), [31] * 4, [big] * 4,
                 31, 32, "wrap to zero")
    assert len(got[2]) == 0 and r.model.stats() == (0, NONE, 32)
    r.drop()


# -------------------------------------------------- projection and filter

def test_projection_and_filter(g):
    """The mfp filters on a val field and projects to a narrower val with a
    MUL field; two input rows that project to the same output consolidate
    in ready and in held."""
    sch = abi.schema(1, 32)  # [ts][x][y][flag]
    mfp = abi.closure(
        [abi.filt(VS, 24, 8, abi.MZ_CMP_GT, 0)], [abi.field(KEY, 0, 8)],
        [abi.field(CP, abi.MZ_COMPUTE_MUL_I64, 8, arg0=8, arg1=16,
                   arg0_src=VS, arg1_src=VS)], abi.schema(1, 8))

    def fn(key, val):
        if i64_at(val, 24) <= 0:
            return None
        return key, wrap(i64_at(val, 8) * i64_at(val, 16)) \
            .to_bytes(8, "little", signed=True)

    n = 500
    i = np.arange(n)
    vals = np.stack([10 + i % 3, i % 4, 3 - i % 4 + (i % 4 == 0) * 2**62,
                     i % 5 - 1], 1).astype(np.int64)
    bounds = [abi.time_bound(GE, VS, 0), abi.time_bound(LT, VS, 0, add=20)]
    r = Rig(g, sch, bounds, mfp=mfp, fn=fn)
    got = r.push(i % 6, vals.view(np.uint8), np.full(n, 10), np.ones(n), 10,
                 12, "mfp")
    assert 0 < len(got[2]) < n / 4 and (got[3] > 1).any()
    assert 0 < r.model.stats()[0] < n / 4
    r.tick(40, "mfp")
    assert r.model.stats()[0] == 0
    r.drop()


# ----------------------------------------------------------------- growth

def test_growth(g):
    """initial_rows = 8, 2k held rows over two pushes, then release all."""
    n = 1000
    i = np.arange(n)
    r = Rig(g, SCH, AB, initial_rows=8)
    r.push(i, ab_vals(np.zeros(n), 100 + i % 50), np.full(n, 1), np.ones(n),
           1, 2, "grow 1")
    r.push(i + n, ab_vals(np.zeros(n), 100 + i % 50), np.full(n, 2),
           np.ones(n), 2, 3, "grow 2")
    assert r.model.stats() == (2 * n, 100, 3)
    got = r.tick(200, "release all")
    assert len(got[2]) == 2 * n and r.model.stats() == (0, NONE, 200)
    r.drop()


# --------------------------------------------------------------- refusals

def test_push_refusals_leave_state_untouched(g):
    from materialize_amd._ffi import MzGpuError
    r = Rig(g, SCH, AB)
    r.push([1, 2], ab_vals([0, 0], [30, 40]), [10, 10], [1, 1], 10, 11,
           "before")
    before = g.temporal_stats(r.op)
    vals = ab_vals([0], [35])
    with pytest.raises(MzGpuError, match="frontier"):
        g.temporal_push(r.op, r.updates([3], vals, [12], [1], 12, 13))
    with pytest.raises(MzGpuError, match="outside"):  # time == upper
        g.temporal_push(r.op, r.updates([3], vals, [12], [1], 11, 12))
    with pytest.raises(MzGpuError, match="outside"):  # time < lower
        g.temporal_push(r.op, r.updates([3], vals, [10], [1], 11, 12))
    with pytest.raises(MzGpuError, match="outside"):  # with a release due
        g.temporal_push(r.op, r.updates([3], vals, [50], [1], 11, 45))
    with pytest.raises(MzGpuError, match="before delta.lower"):
        g.temporal_push(r.op, r.updates([], vals[:0], [], [], 11, 10))
    assert g.temporal_stats(r.op) == before
    r.push([3], vals, [11], [1], 11, 12, "after refusals")
    r.tick(50, "after refusals")
    r.drop()


def test_create_refusals(g):
    """The C layer refuses what abi.temporal_spec refuses (here the spec is
    built by hand, past the Python checks), and a following valid operator
    still matches the model."""
    from materialize_amd._ffi import MzGpuError

    def raw(sch, bounds, mfp=None):
        sp = abi.TemporalSpec()
        sp.in_ = sch
        sp.has_mfp = 0 if mfp is None else 1
        if mfp is not None:
            sp.mfp = mfp
        sp.n_bounds = len(bounds)
        for i, b in enumerate(bounds[:abi.MZ_GPU_MAX_BOUNDS]):
            sp.bounds[i] = b
        sp.until = NONE
        return sp

    flat = AB[0] + AB[1]
    ident_k = [abi.field(KEY, 0, 8)]
    bad = [
        (raw(abi.schema(1, abi.MZ_GPU_VARLEN), flat), "varlen"),
        (raw(SCH, flat, abi.closure([], ident_k, [abi.field(VL, 0, 16)],
                                    SCH)), "MZ_SRC_VAL_LOOKUP"),
        (raw(SCH, flat, abi.closure(
            [], ident_k,
            [abi.field(VS, 0, 8),
             abi.field(CP, abi.MZ_COMPUTE_DIV_I64, 8, arg0=0, arg1=8,
                       arg0_src=VS, arg1_src=VS)], SCH)),
         "MZ_COMPUTE_DIV_I64"),
        (raw(SCH, []), "n_bounds"),
        (raw(SCH, flat * 3), "n_bounds"),
        (raw(SCH, [abi.TimeBound(kind=LOWER, src=VS, off=12, width=8)]),
         "reads past"),
        (raw(SCH, flat, abi.closure([], ident_k, [abi.field(VS, 8, 16)],
                                    SCH)), "reads past"),
        (raw(abi.schema(1, 64), flat, abi.closure(
            [], ident_k, [abi.field(VS, 0, 64), abi.field(VS, 0, 8)],
            abi.schema(1, 72))), "out schema"),
    ]
    for sp, msg in bad:
        with pytest.raises(MzGpuError, match=msg):
            g.temporal_create(sp)
    r = Rig(g, SCH, AB)
    r.push([1], ab_vals([0], [30]), [10], [1], 10, 11, "after refusals")
    r.tick(31, "after refusals")
    r.drop()


def test_render_surface(g):
    op = render.render_temporal_filter(
        g, render.TemporalFilterPlan(abi.temporal_spec(SCH, AB)))
    assert op.stats() == (0, NONE, NONE)
    with pytest.raises(ValueError, match="before the first push"):
        op.advance(5)
    out = op.push(abi.make_updates(np.array([4]), ab_vals([0], [9]), [3],
                                   [2], 3, 4))
    assert out.sorted and out.to_host()[2].tolist() == [3]
    out.release()
    assert op.stats() == (1, 9, 4)
    out = op.advance(10)
    assert out.to_host()[3].tolist() == [-2] and op.stats() == (0, NONE, 10)
    out.release()
    op.drop()
    assert op.op is None


# ------------------------------------------------------------- end to end

def test_sliding_window_feeds_reduce_and_arrangement(g):
    """render_temporal_filter -> render_reduce (COUNT, SUM per key, fed by
    the multi-timestamp reduce_push_dev) over 12 steps of a sliding window
    `mz_now() >= ts AND mz_now() < ts + W` with inserts, deletes and pure
    ticks. After every step the accumulated reduce output equals the CPU
    oracle's reduce over a from-scratch recompute of the rows whose window
    contains now = upper - 1. The released batches also go into an
    arrangement with the push's bounds, and peek_scan as of upper - 1
    returns exactly the live rows: the batches respect [lower, upper)."""
    from pyoracle import OracleCtx
    W = 3
    bounds = [abi.time_bound(GE, VS, 0), abi.time_bound(LT, VS, 0, add=W)]
    tf = render.render_temporal_filter(
        g, render.TemporalFilterPlan(abi.temporal_spec(SCH, bounds)))
    aggs = [abi.Aggregate(func=abi.MZ_AGG_COUNT, off=0, width=8),
            abi.Aggregate(func=abi.MZ_AGG_SUM_I64, off=8, width=8)]
    rspec = abi.reduce_spec(aggs, SCH)
    red = render.render_reduce(g, render.ReducePlan(rspec))
    arr = g.arr_create(SCH)
    rng = np.random.default_rng(7)
    inputs = []   # (key, ts, x, t, d): every input update so far
    alive = []    # inserted in an earlier step, not yet deleted (key, ts, x)
    acc = {}      # accumulated reduce output (key, val bytes) -> diff
    # (lower, upper, is a pure tick)
    steps = [(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 5, 0), (5, 6, 1),
             (6, 7, 0), (7, 8, 0), (8, 11, 1), (11, 12, 0), (12, 14, 0),
             (14, 15, 0), (15, 30, 1)]
    assert len(steps) == 12
    for lower, upper, tick in steps:
        new, fresh = [], []
        if not tick:
            for _ in range(60):
                t = int(rng.integers(lower, upper))
                if alive and rng.random() < 0.35:
                    k, ts, x = alive.pop(int(rng.integers(len(alive))))
                    new.append((k, ts, x, t, -1))
                else:
                    row = (int(rng.integers(8)), t + int(rng.integers(-2, 3)),
                           int(rng.integers(100)))
                    if row[1] < 0:
                        continue
                    fresh.append(row)
                    new.append(row + (t, 1))
        inputs += new
        alive += fresh
        if tick:
            out = tf.advance(upper)
        else:
            out = tf.push(abi.make_updates(
                np.array([r[0] for r in new], np.int64),
                ab_vals([r[1] for r in new], [r[2] for r in new]),
                np.array([r[3] for r in new], np.uint64),
                np.array([r[4] for r in new], np.int64), lower, upper))
        k, v, t, d = out.to_host()
        assert ((t >= lower) & (t < upper)).all()
        if out.n:
            g.arr_insert(arr, out.updates(lower, upper))
            ro = red.push(out.updates(lower, upper))
            rk, rv, _, rd = ro.to_host()
            ro.release()
            rv = rv.reshape(len(rd), -1)
            for j in range(len(rd)):
                key = (int(rk[j]), rv[j].tobytes())
                acc[key] = acc.get(key, 0) + int(rd[j])
        out.release()
        # from scratch: the rows whose window contains now
        now = upper - 1
        live = {}
        for key, ts, x, t, d in inputs:
            if max(t, ts) <= now < ts + W:
                row = (key, ts, x)
                live[row] = live.get(row, 0) + d
        live = {r: m for r, m in live.items() if m}
        assert all(m > 0 for m in live.values())
        rows = sorted(live)
        o = OracleCtx()
        want = {}
        if rows:
            wk, wv, _, wd = o.reduce_push(o.reduce_create(rspec),
                                          abi.make_updates(
                np.array([r[0] for r in rows], np.int64),
                ab_vals([r[1] for r in rows], [r[2] for r in rows]),
                np.zeros(len(rows), np.uint64),
                np.array([live[r] for r in rows], np.int64), 0, 1))
            wv = np.asarray(wv).reshape(len(wd), -1)
            want = {(int(wk[j]), wv[j].tobytes()): int(wd[j])
                    for j in range(len(wd))}
        o.close()
        assert {r: m for r, m in acc.items() if m} == want, \
            f"reduce after [{lower}, {upper})"
        pk, pv, pt, pd = g.peek_scan(arr, now)
        assert pk.tolist() == [r[0] for r in rows], f"peek at {now}"
        same((pv, pd),
             (ab_vals([r[1] for r in rows], [r[2] for r in rows]).ravel(),
              np.array([live[r] for r in rows], np.int64)),
             f"peek at {now}", ("vals", "diffs"))
    assert tf.stats()[0] == 0
    tf.drop()
    red.drop()
