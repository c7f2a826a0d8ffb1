"""Window functions (mz_gpu_window_* / k_window_emit) on the GPU.

Reference: `model_output` below, a naive Python model. It takes the net
counts per (key, val), and per partition repeats every row by its count,
sorts the copies by the order columns with valdomain.canon_val_key as the
tie-break, and evaluates every function at every position from the
definitions in include/mz_gpu.h, by scanning the expanded list. It shares
nothing with the engine (no prefix sums, no searches, no peer-start arrays).

After every push the engine is compared two ways: the push's corrections
equal model(new) - model(old) per time slice, byte for byte and in canonical
order (keys as signed tuples, vals as zero-padded little-endian u64 words,
then time); and the running sum of all corrections equals model(current).
The CPU oracle has no window operator.
"""
import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd import render
from valdomain import canon_val_key

pytestmark = pytest.mark.gpu

PART, TO_CUR = abi.MZ_WF_FRAME_PARTITION, abi.MZ_WF_FRAME_TO_CURRENT
RANKS = (abi.MZ_WF_ROW_NUMBER, abi.MZ_WF_RANK, abi.MZ_WF_DENSE_RANK)


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


# ------------------------------------------------------------ reference

def datum(v, f):
    if f.nullable and v[f.off + f.width] != 0:
        return None
    return int.from_bytes(v[f.off:f.off + f.width], "little", signed=True)


def slot(f, x):
    if f.func in RANKS:
        return x.to_bytes(8, "little", signed=True)
    if x is None:
        return bytes(8) + b"\x01"
    return x.to_bytes(8, "little", signed=True) + b"\x00"


def eval_partition(rows, order, funcs):
    """rows: [(val bytes, count > 0)] of one partition. -> [val ++ slots]
    of every position of the expanded, ordered sequence."""
    def ocols(v):
        return tuple(
            (-1 if desc else 1)
            * int.from_bytes(v[off:off + w], "little", signed=True)
            for off, w, desc in order)

    E = sorted((v for v, c in rows for _ in range(c)),
               key=lambda v: (ocols(v), canon_val_key(v)))
    M = len(E)
    peers = [ocols(v) for v in E]
    out = []
    for p in range(M):
        mine = [q for q in range(M) if peers[q] == peers[p]]
        row = E[p]
        for f in funcs:
            if f.func == abi.MZ_WF_ROW_NUMBER:
                x = p + 1
            elif f.func == abi.MZ_WF_RANK:
                x = mine[0] + 1
            elif f.func == abi.MZ_WF_DENSE_RANK:
                x = 1 + len(set(peers[:mine[0]]))
            elif f.func in (abi.MZ_WF_LAG, abi.MZ_WF_LEAD):
                q = p - f.offset if f.func == abi.MZ_WF_LAG else p + f.offset
                if 0 <= q < M:
                    x = datum(E[q], f)
                else:
                    x = f.dflt if f.has_default else None
            elif f.func == abi.MZ_WF_FIRST_VALUE:
                x = datum(E[0], f)
            else:
                x = datum(E[M - 1 if f.frame == PART else mine[-1]], f)
            row = row + slot(f, x)
        out.append(row)
    return out


def model_output(net, order, funcs, keys=None):
    """{(key, out val): count} of the partitions in `keys` (None: all)."""
    parts = {}
    for (k, v), c in net.items():
        if c and (keys is None or k in keys):
            assert c > 0
            parts.setdefault(k, []).append((v, c))
    out = {}
    for k, rows in parts.items():
        for ov in eval_partition(rows, order, funcs):
            out[(k, ov)] = out.get((k, ov), 0) + 1
    return out


def cols_of(rows, kw):
    rows = sorted(rows, key=lambda r: (r[0], canon_val_key(r[1]), r[2]))
    return (np.array([x for r in rows for x in r[0]], np.int64),
            np.frombuffer(b"".join(r[1] for r in rows), np.uint8),
            np.array([r[2] for r in rows], np.uint64),
            np.array([r[3] for r in rows], np.int64))


def same(got, want, what):
    for a, b, col in zip(got, want, ("keys", "vals", "times", "diffs")):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype.itemsize == b.dtype.itemsize, f"{what}: {col} dtype"
        np.testing.assert_array_equal(
            np.ascontiguousarray(a).view(np.uint8),
            np.ascontiguousarray(b).view(np.uint8), err_msg=f"{what}: {col}")


class Rig:
    """One window operator beside the model's net counts."""

    def __init__(self, g, in_schema, order, funcs):
        self.g, self.order, self.funcs = g, order, funcs
        self.kw, self.vb = in_schema.key_words, in_schema.val_bytes
        self.spec = abi.window_spec(in_schema, order, funcs)
        self.ovb = self.spec.out.val_bytes
        self.op = g.window_create(self.spec)
        self.net, self.acc = {}, {}

    def drop(self):
        self.g.window_drop(self.op)

    def updates(self, rows, lower, upper):
        """rows: [(key tuple, val bytes, time, diff)]."""
        keys = np.array([x for r in rows for x in r[0]], np.int64)
        vals = np.frombuffer(b"".join(r[1] for r in rows), np.uint8)
        return abi.make_updates(
            keys, vals if self.vb else None,
            np.array([r[2] for r in rows], np.uint64),
            np.array([r[3] for r in rows], np.int64), lower, upper)

    def expect(self, rows):
        """model(new) - model(old) per time slice, in time order."""
        want = []
        for t in sorted({r[2] for r in rows}):
            touched = {r[0] for r in rows if r[2] == t}
            old = model_output(self.net, self.order, self.funcs, touched)
            for k, v, rt, d in rows:
                if rt == t:
                    self.net[(k, v)] = self.net.get((k, v), 0) + d
            new = model_output(self.net, self.order, self.funcs, touched)
            for r in set(old) | set(new):
                d = new.get(r, 0) - old.get(r, 0)
                if d:
                    want.append((r[0], r[1], t, d))
        return want

    def push(self, rows, lower, upper, what):
        want = self.expect(rows)
        got = self.g.window_push(self.op, self.updates(rows, lower, upper))
        same(got, cols_of(want, self.kw), what)
        k, v, t, d = got
        for i in range(len(t)):
            r = (tuple(int(x) for x in k[i * self.kw:(i + 1) * self.kw]),
                 bytes(v[i * self.ovb:(i + 1) * self.ovb]))
            self.acc[r] = self.acc.get(r, 0) + int(d[i])
        assert {r: c for r, c in self.acc.items() if c} == \
            model_output(self.net, self.order, self.funcs), \
            f"{what}: running sum"
        return want


def i32(x):
    return int(x).to_bytes(4, "little", signed=True)


def i64(x):
    return int(x).to_bytes(8, "little", signed=True)


def nullable64(x):
    """An i64 datum and its null byte; garbage under a NULL."""
    return b"\xa5" * 8 + b"\x01" if x is None else i64(x) + b"\x00"


# ------------------------------------------------------ boundary crossing
# val: a i32 @0, b i32 @4, x i64 @8 null @16, y i32 @17
AB = abi.schema(1, 21)
AB_ORDER = [(0, 4, True), (4, 4, False)]


def ab_row(a, b, x, y):
    return i32(a) + i32(b) + nullable64(x) + i32(y)


def X(**kw):
    return dict(off=8, width=8, nullable=1, **kw)


def Y(**kw):
    return dict(off=17, width=4, **kw)


AB_SPECS = {
    "expanding": lambda: [abi.wf_row_number(), abi.wf_rank(),
                          abi.wf_lag(k=1, **X()),
                          abi.wf_last_value(frame=TO_CUR, **X())],
    "expanding2": lambda: [abi.wf_dense_rank(),
                           abi.wf_lead(k=2, default=7, **Y()),
                           abi.wf_first_value(**X()),
                           abi.wf_last_value(frame=PART, **Y())],
    # one output row per input row: more than one block of rows
    "per_row": lambda: [abi.wf_rank(), abi.wf_dense_rank(),
                        abi.wf_first_value(**Y()),
                        abi.wf_last_value(frame=TO_CUR, **X())],
}


def big_partition(rng, key, n):
    """n distinct rows of one partition, counts 1..3; a negative and
    positive, (a, b) often tied, a few NULL x."""
    rows = []
    for i in range(n):
        x = None if i % 17 == 3 else int(rng.integers(-2**40, 2**40)) * n + i
        rows.append(((key,), ab_row(int(rng.integers(-6, 6)),
                                    int(rng.integers(-3, 3)), x,
                                    int(rng.integers(-2**31, 2**31))),
                     0, int(rng.integers(1, 4))))
    return rows


@pytest.mark.parametrize("name", sorted(AB_SPECS))
def test_boundary_crossing(g, name):
    rng = np.random.default_rng(7)
    rig = Rig(g, AB, AB_ORDER, AB_SPECS[name]())
    rows = big_partition(rng, 5, 300)
    for k in range(12):
        rows += big_partition(rng, 100 + k, 1 + k % 4)
    assert sum(r[3] for r in rows if r[0] == (5,)) > 512  # > 2 blocks
    rig.push(rows, 0, 1, f"{name}: load")
    # retract rows of the large partition and of small ones, add others
    churn = [(k, v, 1, -1) for k, v, _, d in rows[40:300:37]]
    churn += [(k, v, 1, -d) for k, v, _, d in rows[300:306]]
    churn += [(k, v, 1, d) for k, v, _, d in big_partition(rng, 5, 9)]
    rig.push(churn, 1, 2, f"{name}: churn")
    rig.drop()


# ------------------------------------------------------------------ peers

def test_peers(g):
    """Few distinct order values: RANK, DENSE_RANK and ROW_NUMBER all
    differ, and LAST_VALUE's two frames differ over peers whose datums
    differ."""
    rng = np.random.default_rng(11)
    rows = []
    for key in (1, 2, 3):
        for i in range(40):
            rows.append(((key,), ab_row(int(rng.integers(-2, 2)), 0,
                                        1000 * key + i, i), 0,
                         int(rng.integers(1, 3))))
    specs = [
        [abi.wf_row_number(), abi.wf_rank(), abi.wf_dense_rank(),
         abi.wf_last_value(frame=TO_CUR, **X())],
        [abi.wf_rank(), abi.wf_dense_rank(),
         abi.wf_last_value(frame=TO_CUR, **X()),
         abi.wf_last_value(frame=PART, **X())],
    ]
    for n, funcs in enumerate(specs):
        rig = Rig(g, AB, [(0, 4, True)], funcs)
        want = rig.push(rows, 0, 1, f"peers spec {n}")
        if n == 0:  # some position has three different numbers
            assert any(len({r[1][21:29], r[1][29:37], r[1][37:45]}) == 3
                       for r in want)
        else:
            assert any(r[1][37:46] != r[1][46:55] for r in want)  # frames
        rig.drop()


def test_no_order_is_one_peer_group(g):
    rows = [((k,), ab_row(a, 0, 10 * a, a), 0, 1 + a % 2)
            for k in (1, 2) for a in range(-3, 4)]
    rig = Rig(g, AB, [], [abi.wf_rank(), abi.wf_dense_rank(),
                          abi.wf_last_value(frame=TO_CUR, **X()),
                          abi.wf_row_number()])
    want = rig.push(rows, 0, 1, "n_order = 0")
    # every position has rank 1, dense rank 1 and the x of the partition's
    # last row, which in canonical val order is a = -1 (0xFFFFFFFF)
    assert all(r[1][21:37] == i64(1) + i64(1) for r in want)
    assert {r[1][37:46] for r in want} == {i64(-10) + b"\x00"}
    rig.drop()


# --------------------------------------------------------- LAG/LEAD edges
# val: x i64 @0 null @8, y i32 @9
XY = abi.schema(1, 13)


def xy_row(x, y):
    return nullable64(x) + i32(y)


def test_lag_lead_edges(g):
    fx = dict(off=0, width=8, nullable=1)
    fy = dict(off=9, width=4)
    specs = [
        [abi.wf_lag(k=0, **fx), abi.wf_lag(k=1, **fx),
         abi.wf_lead(k=1000, default=-9, **fx), abi.wf_lead(k=1, **fy)],
        [abi.wf_lag(k=1, default=42, **fx), abi.wf_lead(k=1000, **fx),
         abi.wf_lead(k=0, **fy), abi.wf_lag(k=2, default=-2**63, **fy)],
    ]
    rows = [((1,), xy_row(10, -1), 0, 1),
            ((1,), xy_row(None, 0), 0, 2),
            ((1,), xy_row(-2**63, 1), 0, 3),   # LAG 1 lands in its own copy
            ((1,), xy_row(None, 2), 0, 1),
            ((1,), xy_row(2**63 - 1, -2**31), 0, 1),
            ((2,), xy_row(77, 5), 0, 1)]       # a single-row partition
    for n, funcs in enumerate(specs):
        rig = Rig(g, XY, [(9, 4, False)], funcs)
        want = rig.push(rows, 0, 1, f"lag/lead spec {n}")
        assert len(want) == 9
        if n == 0:
            # k = 0 of a NULL is the canonical NULL slot, whatever lies
            # under the input's null byte
            nulls = [r for r in want if r[1][8] == 1]
            assert len(nulls) == 3
            assert all(r[1][13:22] == bytes(8) + b"\x01" for r in nulls)
            # k beyond the partition: the literal default everywhere
            assert all(r[1][31:40] == i64(-9) + b"\x00" for r in want)
        rig.drop()


# ------------------------------------------------------------------ churn

def v8(x):
    return i64(x)


def test_churn(g):
    """Eight steps of insert / retract churn that never goes negative,
    then the directed events."""
    rng = np.random.default_rng(3)
    rig = Rig(g, abi.schema(1, 8), [(0, 8, False)],
              [abi.wf_row_number(), abi.wf_lag(0, 8, 1)])
    for t in range(8):
        rows, step = [], {}
        for _ in range(60):
            r = ((int(rng.integers(0, 6)),), v8(int(rng.integers(-20, 20))))
            cur = rig.net.get(r, 0) + step.get(r, 0)
            if cur > 0 and rng.random() < 0.45:
                d = -int(rng.integers(1, cur + 1))
            else:
                d = int(rng.integers(1, 3))
            step[r] = step.get(r, 0) + d
            rows.append((r[0], r[1], t, d))
        rig.push(rows, t, t + 1, f"churn step {t}")
    # a fresh partition, then retract its middle row: every later row is
    # renumbered and the successor's LAG changes
    rig.push([((9,), v8(x), 8, 1) for x in (1, 2, 3, 4, 5)], 8, 9, "insert")
    want = rig.push([((9,), v8(3), 9, -1)], 9, 10, "retract the middle")
    assert sorted(r[3] for r in want) == [-1, -1, -1, 1, 1]
    # a push that nets to no change
    want = rig.push([((9,), v8(7), 10, 1), ((9,), v8(7), 10, -1),
                     ((9,), v8(1), 10, -1), ((9,), v8(1), 10, 1)], 10, 11,
                    "no net change")
    assert want == []
    # retracting a whole partition yields only retractions
    want = rig.push([((9,), v8(x), 11, -1) for x in (1, 2, 4, 5)], 11, 12,
                    "retract the partition")
    assert len(want) == 4 and all(r[3] == -1 for r in want)
    rig.drop()


def test_multi_timestamp(g):
    """Two timestamps in one push touch the same partition: corrections at
    both times, the second time's old being the first time's new."""
    rig = Rig(g, abi.schema(1, 8), [(0, 8, True)],
              [abi.wf_rank(), abi.wf_lead(0, 8, 1, default=0)])
    rows = [((1,), v8(10), 0, 1), ((1,), v8(30), 0, 2), ((2,), v8(5), 0, 1),
            ((1,), v8(20), 1, 1), ((1,), v8(30), 1, -1), ((3,), v8(6), 1, 1)]
    want = rig.push(rows, 0, 2, "two timestamps")
    assert {r[2] for r in want} == {0, 1}
    # the t = 1 slice retracts rows the t = 0 slice produced
    at0 = {(r[0], r[1]) for r in want if r[2] == 0 and r[3] > 0}
    assert any((r[0], r[1]) in at0 for r in want if r[2] == 1 and r[3] < 0)
    rig.drop()


# -------------------------------------------------------- expansion rule

def test_huge_multiplicity_without_expansion(g):
    """RANK, DENSE_RANK and FIRST_VALUE do not differ between the copies of
    a row: one out row per input row, diff = the multiplicity."""
    spec = abi.window_spec(abi.schema(1, 8), [(0, 8, False)],
                           [abi.wf_rank(), abi.wf_dense_rank(),
                            abi.wf_first_value(0, 8)])
    op = g.window_create(spec)
    u = abi.make_updates(
        np.array([4, 4], np.int64),
        np.frombuffer(v8(1) + v8(2), np.uint8),
        np.zeros(2, np.uint64), np.array([2**40, 3], np.int64), 0, 1)
    got = g.window_push(op, u)
    want = [((4,), v8(1) + i64(1) + i64(1) + i64(1) + b"\x00", 0, 2**40),
            ((4,), v8(2) + i64(2**40 + 1) + i64(2) + i64(1) + b"\x00", 0, 3)]
    same(got, cols_of(want, 1), "2^40 copies")
    g.window_drop(op)


@pytest.mark.parametrize("counts", [(2**40,), (2**30, 2**30)])
def test_expansion_limit(g, counts):
    """ROW_NUMBER expands: 2^31 positions or more fail the push."""
    from materialize_amd._ffi import MzGpuError
    spec = abi.window_spec(abi.schema(1, 8), [(0, 8, False)],
                           [abi.wf_row_number()])
    op = g.window_create(spec)
    n = len(counts)
    u = abi.make_updates(
        np.full(n, 4, np.int64),
        np.frombuffer(b"".join(v8(i) for i in range(n)), np.uint8),
        np.zeros(n, np.uint64), np.array(counts, np.int64), 0, 1)
    with pytest.raises(MzGpuError,
                       match=r"window: expanded partition exceeds 2\^31 rows"):
        g.window_push(op, u)
    g.window_drop(op)


@pytest.mark.parametrize("funcs", [
    lambda: [abi.wf_row_number()], lambda: [abi.wf_rank()]])
def test_negative_net_count(g, funcs):
    from materialize_amd._ffi import MzGpuError
    spec = abi.window_spec(abi.schema(1, 8), [(0, 8, False)], funcs())
    op = g.window_create(spec)
    u = abi.make_updates(np.array([1, 1], np.int64),
                         np.frombuffer(v8(1) + v8(2), np.uint8),
                         np.zeros(2, np.uint64),
                         np.array([2, -1], np.int64), 0, 1)
    with pytest.raises(MzGpuError, match="negative multiplicities in window"):
        g.window_push(op, u)
    g.window_drop(op)


def test_create_refusals_reach_the_c_layer(g):
    """The C layer checks a spec itself: one that abi.window_spec would
    have refused, built by hand."""
    from materialize_amd._ffi import MzGpuError
    spec = abi.window_spec(abi.schema(1, 8), [], [abi.wf_rank()])
    spec.out.val_bytes = 17
    with pytest.raises(MzGpuError, match="window: out schema must be"):
        g.window_create(spec)
    spec = abi.window_spec(abi.schema(1, 8), [], [abi.wf_lag(0, 8)])
    spec.funcs[0].off = 1
    with pytest.raises(MzGpuError, match="window: func 0 reads past"):
        g.window_create(spec)


def test_empty_val_row_number(g):
    """in.val_bytes = 0 and two key words: multiplicity 3 is three rows."""
    rig = Rig(g, abi.schema(2, 0), [], [abi.wf_row_number()])
    want = rig.push([((7, -1), b"", 0, 3), ((7, -2), b"", 0, 1)], 0, 1,
                    "vb = 0")
    assert sorted((r[0], r[1]) for r in want) == \
        [((7, -2), i64(1)), ((7, -1), i64(1)), ((7, -1), i64(2)),
         ((7, -1), i64(3))]
    rig.drop()


# ------------------------------------------------------------ composition

def test_lag_slot_feeds_an_mfp(g):
    """delta to the previous reading: the window's LAG slot read by
    mz_gpu_mfp as COL width 8 nullable."""
    in_s = abi.schema(1, 8)
    wspec = abi.window_spec(in_s, [(0, 8, False)], [abi.wf_lag(0, 8, 1)])
    assert wspec.out.val_bytes == 17
    VS = abi.MZ_SRC_VAL_STREAM
    x, lag = abi.x_col(VS, 0), abi.x_col(VS, 8, 8, 1)
    mspec = abi.mfp_spec(wspec.out, abi.schema(1, 8), [
        abi.x_filter(~abi.x_is_null(lag)),
        abi.x_out_key(abi.x_col(abi.MZ_SRC_KEY, 0), 0),
        abi.x_out_val(x - lag, 0, 8)])
    win = render.render_window(g, render.WindowPlan(wspec))
    mfp = render.render_mfp(g, render.MfpPlan(mspec))
    readings = {1: [5, 9, 10, 40], 2: [-3], 3: [100, 50]}
    rows = [((k,), v8(x), 0, 1) for k, xs in readings.items() for x in xs]
    u = abi.make_updates(np.array([r[0][0] for r in rows], np.int64),
                         np.frombuffer(b"".join(r[1] for r in rows),
                                       np.uint8),
                         np.zeros(len(rows), np.uint64),
                         np.ones(len(rows), np.int64), 0, 1)
    wout = win.push(u)
    assert wout.n == len(rows) and wout.schema == (1, 17)
    mout = mfp.push(wout.updates(0, 1))
    got = mout.to_host()
    assert mout.errs_to_host()[0].size == 0
    want = []
    for k, xs in readings.items():
        xs = sorted(xs)
        want += [((k,), v8(b - a), 0, 1) for a, b in zip(xs, xs[1:])]
    same(got, cols_of(want, 1), "x - lag")
    mout.release()
    wout.release()
    win.drop()
