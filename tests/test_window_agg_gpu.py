"""Window aggregates (SUM / COUNT / MIN / MAX OVER a frame) on the GPU.

Reference: `model_output` below, a naive Python model. It takes the net
counts per (key, val), and per partition repeats every row by its count,
sorts the copies by the order columns with valdomain.canon_val_key as the
tie-break, and at every position materialises the frame of include/mz_gpu.h
as a Python slice of the expanded list and applies sum / len / min / max
with Python ints. No prefix sums, no searches, no 128-bit limbs: nothing of
the engine's method.

After every push the engine is compared two ways, as test_window_gpu.py
does: the push's corrections equal model(new) - model(old) per time slice,
byte for byte and in canonical order; and the running sum of all
corrections equals model(current).
"""
import numpy as np
import pytest

from materialize_amd import _abi as abi
from valdomain import canon_val_key

pytestmark = pytest.mark.gpu

TO_CUR, PART, ROWS = (abi.MZ_WF_FRAME_TO_CURRENT, abi.MZ_WF_FRAME_PARTITION,
                      abi.MZ_WF_FRAME_ROWS)
UP, CUR, UF = abi.UNBOUNDED_PRECEDING, abi.CURRENT_ROW, abi.UNBOUNDED_FOLLOWING
P, F = abi.preceding, abi.following
I64_SLOTS = (abi.MZ_WF_ROW_NUMBER, abi.MZ_WF_RANK, abi.MZ_WF_DENSE_RANK,
             abi.MZ_WF_COUNT)
AGGS = (abi.MZ_WF_SUM, abi.MZ_WF_COUNT, abi.MZ_WF_MIN, abi.MZ_WF_MAX)


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


# ------------------------------------------------------------ reference

def datum(v, f):
    if f.width == 0:
        return 1  # COUNT(*): every position counts
    if f.nullable and v[f.off + f.width] != 0:
        return None
    return int.from_bytes(v[f.off:f.off + f.width], "little", signed=True)


def slot(f, x):
    if f.func in I64_SLOTS:
        return x.to_bytes(8, "little", signed=True)
    if x is None:
        return bytes(8) + b"\x01"
    return x.to_bytes(8, "little", signed=True) + b"\x00"


def frame_slice(f, xs, p, last_peer):
    """The frame of position p as a slice of the partition's datums xs."""
    M = len(xs)
    if f.frame == TO_CUR:
        return xs[:last_peer + 1]
    if f.frame == PART:
        return xs[:]
    sk, ek = f.bounds & 15, f.bounds >> 4
    a = {abi.MZ_WB_UNBOUNDED_PRECEDING: 0, abi.MZ_WB_PRECEDING: p - f.offset,
         abi.MZ_WB_CURRENT_ROW: p, abi.MZ_WB_FOLLOWING: p + f.offset}[sk]
    b = {abi.MZ_WB_PRECEDING: p - f.end_offset, abi.MZ_WB_CURRENT_ROW: p,
         abi.MZ_WB_FOLLOWING: p + f.end_offset,
         abi.MZ_WB_UNBOUNDED_FOLLOWING: M - 1}[ek]
    a, b = max(a, 0), min(b, M - 1)
    return xs[a:b + 1] if a <= b else []


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
    first_peer, last_peer = [0] * M, [M - 1] * M
    for q in range(1, M):
        first_peer[q] = first_peer[q - 1] if peers[q] == peers[q - 1] else q
    for q in range(M - 2, -1, -1):
        last_peer[q] = last_peer[q + 1] if peers[q] == peers[q + 1] else q
    xs = [[datum(v, f) for v in E] for f in funcs]
    out = []
    for p in range(M):
        row = E[p]
        for f, x_of in zip(funcs, xs):
            if f.func in AGGS:
                fr = [x for x in frame_slice(f, x_of, p, last_peer[p])
                      if x is not None]
                if f.func == abi.MZ_WF_COUNT:
                    x = len(fr)
                elif not fr:
                    x = None
                else:
                    x = {abi.MZ_WF_SUM: sum, abi.MZ_WF_MIN: min,
                         abi.MZ_WF_MAX: max}[f.func](fr)
            elif f.func == abi.MZ_WF_ROW_NUMBER:
                x = p + 1
            elif f.func == abi.MZ_WF_RANK:
                x = first_peer[p] + 1
            elif f.func == abi.MZ_WF_DENSE_RANK:
                x = len(set(peers[:first_peer[p] + 1]))
            elif f.func in (abi.MZ_WF_LAG, abi.MZ_WF_LEAD):
                q = p - f.offset if f.func == abi.MZ_WF_LAG else p + f.offset
                if 0 <= q < M:
                    x = x_of[q]
                else:
                    x = f.dflt if f.has_default else None
            elif f.func == abi.MZ_WF_FIRST_VALUE:
                x = x_of[0]
            else:
                x = x_of[M - 1 if f.frame == PART else last_peer[p]]
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


def updates_of(rows, vb, lower, upper):
    """rows: [(key tuple, val bytes, time, diff)]."""
    keys = np.array([x for r in rows for x in r[0]], np.int64)
    vals = np.frombuffer(b"".join(r[1] for r in rows), np.uint8)
    return abi.make_updates(
        keys, vals if vb else None,
        np.array([r[2] for r in rows], np.uint64),
        np.array([r[3] for r in rows], np.int64), lower, upper)


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
        got = self.g.window_push(self.op,
                                 updates_of(rows, self.vb, lower, upper))
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


NULL_SLOT = bytes(8) + b"\x01"

# val: a i32 @0, b i32 @4, x i64 @8 null @16, y i32 @17
AB = abi.schema(1, 21)
AB_ORDER = [(0, 4, True), (4, 4, False)]
X = dict(off=8, width=8, nullable=1)
Y = dict(off=17, width=4)


def ab_row(a, b, x, y):
    return i32(a) + i32(b) + nullable64(x) + i32(y)


# ------------------------------------------------- frames across the tile
# name -> builder keywords, and whether MIN / MAX may take the frame (one
# end unbounded)
FRAMES = {
    "1p_1f": (dict(start=P(1), end=F(1)), False),
    "2p_cur": (dict(start=P(2), end=CUR), False),
    "cur_uf": (dict(start=CUR, end=UF), True),
    "2f_3f": (dict(start=F(2), end=F(3)), False),     # empty at the tail
    "3p_5p": (dict(start=P(3), end=P(5)), False),     # always empty
    "up_uf": (dict(start=UP, end=UF), True),          # does not expand
    "to_current": (dict(frame=TO_CUR), True),
    "partition": (dict(frame=PART), True),
    "up_2f": (dict(start=UP, end=F(2)), True),
    "2p_uf": (dict(start=P(2), end=UF), True),
}


def sized_partition(rng, key, size):
    """Distinct rows of one partition whose counts, 2..5, sum to `size` (the
    last row takes the remainder); (a, b) often tied, x negative and
    positive with some NULLs (runs of them too), y a negative-heavy i32."""
    rows, left, i = [], size, 0
    while left:
        m = min(left, int(rng.integers(2, 6)))
        x = None if i % 11 in (3, 4, 5) else int(rng.integers(-2**40, 2**40))
        rows.append(((key,), ab_row(int(rng.integers(-4, 4)),
                                    int(rng.integers(-2, 2)), x,
                                    int(rng.integers(-2**31, 2**20))),
                     0, m))
        left -= m
        i += 1
    # distinct vals: y carries the row number in its low bits
    return [(k, v[:17] + i32((int.from_bytes(v[17:], "little", signed=True)
                              & ~0x3FF) | j), t, m)
            for j, (k, v, t, m) in enumerate(rows)]


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frames_across_the_emit_tile(g, name):
    """Three partitions in one snapshot with expanded sizes 255, 257 and 1:
    the global prefixes must not leak from one partition into the next, and
    the 256-row emit tile ends inside a partition. Counts of 2..5 put the
    ends of a ROWS frame in the middle of a row's copies."""
    kw, ext_ok = FRAMES[name]
    rng = np.random.default_rng(5)
    funcs = [abi.wf_sum(**X, **kw), abi.wf_count(**X, **kw),
             abi.wf_count(**kw)]
    funcs.append(abi.wf_min(**X, **kw) if ext_ok else abi.wf_sum(**Y, **kw))
    rig = Rig(g, AB, AB_ORDER, funcs)
    rows = (sized_partition(rng, 1, 255) + sized_partition(rng, 2, 257)
            + sized_partition(rng, 3, 1))
    assert [sum(r[3] for r in rows if r[0] == (k,)) for k in (1, 2, 3)] == \
        [255, 257, 1]
    want = rig.push(rows, 0, 1, f"{name}: load")
    expands = any(abi.wf_expands(f) for f in funcs)
    assert expands == (name not in ("up_uf", "to_current", "partition"))
    assert sum(r[3] for r in want) == 513
    if not expands:
        assert len(want) == len(rows)  # one out row per input row, diff m
    # retractions (one copy of some rows, all copies of others) change the
    # frames of rows they do not touch
    churn = [(k, v, 1, -1) for k, v, _, m in rows[5:120:9]]
    churn += [(k, v, 1, -m) for k, v, _, m in rows[121:130]]
    rig.push(churn, 1, 2, f"{name}: churn")
    rig.drop()


@pytest.mark.parametrize("func", ["max_x", "min_y", "max_y"])
@pytest.mark.parametrize("name", ["up_2f", "2p_uf", "to_current"])
def test_extremum_from_either_end(g, name, func):
    """MAX as well as MIN, over the nullable i64 and the negative i32, with
    the frame anchored at the partition's start and at its end."""
    kw, _ = FRAMES[name]
    rng = np.random.default_rng(9)
    f = {"max_x": abi.wf_max(**X, **kw), "min_y": abi.wf_min(**Y, **kw),
         "max_y": abi.wf_max(**Y, **kw)}[func]
    rig = Rig(g, AB, AB_ORDER, [f, abi.wf_count(**X, **kw)])
    rows = sized_partition(rng, 1, 70) + sized_partition(rng, 2, 33)
    rig.push(rows, 0, 1, f"{name} {func}: load")
    rig.push([(k, v, 1, -m) for k, v, _, m in rows[3:12]], 1, 2,
             f"{name} {func}: retract")
    rig.drop()


# ------------------------------------------------------------------ peers

@pytest.mark.parametrize("order", [[], [(0, 4, True)], [(0, 4, False)]],
                         ids=["no_order", "desc", "asc"])
def test_to_current_includes_the_peers(g, order):
    """Peer groups of several rows: the default frame runs to the end of
    the peer group, so peers share a value; with n_order == 0 the whole
    partition is one peer group and TO_CURRENT equals PARTITION."""
    rng = np.random.default_rng(13)
    rows = [((key,), ab_row(int(rng.integers(-2, 2)), 0,
                            None if i % 7 == 2 else 1000 * key + i, -i), 0,
             int(rng.integers(1, 4)))
            for key in (1, 2, 3) for i in range(30)]
    funcs = [abi.wf_sum(**X), abi.wf_count(**X), abi.wf_min(**Y),
             abi.wf_sum(frame=PART, **X)]
    rig = Rig(g, AB, order, funcs)
    want = rig.push(rows, 0, 1, "peers")
    assert len(want) == len(rows)  # nothing here expands
    if not order:
        assert all(r[1][21:30] == r[1][47:56] for r in want)
    else:
        assert any(r[1][21:30] != r[1][47:56] for r in want)
        # rows with one `a` are peers: one running sum per (key, a)
        sums = {}
        for r in want:
            sums.setdefault((r[0], r[1][:4]), set()).add(r[1][21:30])
        assert all(len(s) == 1 for s in sums.values())
        assert len(sums) > 3
    rig.drop()


# ------------------------------------------------------------------ NULLs
# val: x i64 @0 null @8, y i32 @9
XY = abi.schema(1, 13)
FX = dict(off=0, width=8, nullable=1)
FY = dict(off=9, width=4)


def xy_row(x, y):
    return nullable64(x) + i32(y)


def test_null_frames(g):
    """A frame of only NULLs: SUM / MIN / MAX NULL (canonical slot),
    COUNT(x) 0, COUNT(*) the frame length. Partition 2 holds only NULLs."""
    kw = dict(start=P(1), end=F(1))
    rows = [((1,), xy_row(None, 0), 0, 2), ((1,), xy_row(None, 1), 0, 2),
            ((1,), xy_row(7, 2), 0, 1), ((1,), xy_row(None, 3), 0, 3),
            ((2,), xy_row(None, 0), 0, 2), ((2,), xy_row(None, 1), 0, 1)]
    for n, funcs in enumerate([
            [abi.wf_sum(**FX, **kw), abi.wf_count(**FX, **kw),
             abi.wf_count(**kw)],
            [abi.wf_min(**FX, start=UP, end=F(1)),
             abi.wf_max(**FX, start=P(1), end=UF), abi.wf_count(**kw)],
            [abi.wf_sum(**FX), abi.wf_max(frame=PART, **FX),
             abi.wf_count(frame=PART, **FX)]]):
        rig = Rig(g, XY, [(9, 4, False)], funcs)
        want = rig.push(rows, 0, 1, f"nulls spec {n}")
        p2 = [r for r in want if r[0] == (2,)]
        if n == 0:
            assert len(want) == 11
            # position 0 of partition 1: frame E[0..1], two NULLs
            first = [r for r in want if r[0] == (1,) and r[1][9:13] == i32(0)]
            assert {r[1][13:] for r in first} == \
                {NULL_SLOT + i64(0) + i64(2), NULL_SLOT + i64(0) + i64(3)}
            assert all(r[1][13:30] == NULL_SLOT + i64(0) for r in p2)
            assert sorted(r[1][30:38] for r in p2 for _ in range(r[3])) == \
                [i64(2), i64(2), i64(3)]
        elif n == 1:
            assert all(r[1][13:31] == NULL_SLOT + NULL_SLOT for r in p2)
        else:
            assert len(want) == len(rows)
            assert all(r[1][13:] == NULL_SLOT + NULL_SLOT + i64(0)
                       for r in p2)
        rig.drop()


# ---------------------------------------------------------------- 128 bits

def big_rows():
    """Per partition six rows of x = +-2^62, three copies each: a one-row
    frame's sum fits an i64, the running prefix (up to 18 * 2^62) does not,
    and partition 2's prefix starts beyond 2^64."""
    return [((key,), xy_row(sign * 2**62, j), 0, 3)
            for key, sign in ((1, 1), (2, -1), (3, 1)) for j in range(6)]


def test_sums_beyond_int64_inside_the_prefix(g):
    funcs = [abi.wf_sum(**FX, start=CUR, end=CUR),
             abi.wf_sum(**FY, start=P(1), end=F(1)),
             abi.wf_max(**FX, start=CUR, end=UF),
             abi.wf_count(**FX, start=UP, end=CUR)]
    rig = Rig(g, XY, [(9, 4, False)], funcs)
    want = rig.push(big_rows(), 0, 1, "2^62")
    assert {r[1][13:22] for r in want if r[0] == (2,)} == \
        {i64(-2**62) + b"\x00"}
    # one more copy of the extreme: still a one-row frame
    rig.push([((1,), xy_row(2**62, 0), 1, 1),
              ((2,), xy_row(-2**62, 5), 1, -2)], 1, 2, "2^62 churn")
    rig.drop()


@pytest.mark.parametrize("kw", [dict(frame=PART), dict(start=UP, end=CUR),
                                dict(start=P(1), end=CUR)],
                         ids=["partition", "running", "two_rows"])
def test_sum_out_of_int64_range_fails_the_push(g, kw):
    """The same data under a frame whose sum leaves int64 (two copies of
    2^62 already do): the push fails with the range message, and returns."""
    from materialize_amd._ffi import MzGpuError
    spec = abi.window_spec(XY, [(9, 4, False)],
                           [abi.wf_sum(**FX, **kw), abi.wf_count()])
    op = g.window_create(spec)
    with pytest.raises(MzGpuError, match="window: SUM out of int64 range"):
        g.window_push(op, updates_of(big_rows(), 13, 0, 1))
    g.window_drop(op)


def test_sum_at_the_int64_edges(g):
    """Frame sums of exactly 2^63 - 1 and -2^63 are in range."""
    rows = [((1,), xy_row(2**62, 0), 0, 1), ((1,), xy_row(2**62 - 1, 1), 0, 1),
            ((2,), xy_row(-2**62, 0), 0, 2)]
    rig = Rig(g, XY, [(9, 4, False)],
              [abi.wf_sum(frame=PART, **FX), abi.wf_sum(**FX)])
    want = rig.push(rows, 0, 1, "edges")
    assert {r[1][13:22] for r in want} == \
        {i64(2**63 - 1) + b"\x00", i64(-2**63) + b"\x00"}
    rig.drop()


def test_int32_datums_sign_extend(g):
    rows = [((1,), xy_row(0, -2**31), 0, 2), ((1,), xy_row(1, -1), 0, 3),
            ((1,), xy_row(2, 5), 0, 1)]
    rig = Rig(g, XY, [(0, 8, False)],
              [abi.wf_sum(**FY), abi.wf_min(frame=PART, **FY),
               abi.wf_max(**FY), abi.wf_sum(**FY, start=CUR, end=CUR)])
    want = rig.push(rows, 0, 1, "i32")
    assert sorted(r[1][13:22] for r in want) == \
        sorted(i64(s) + b"\x00" for s in (-2**32, -2**32 - 3, -2**32 + 2))
    assert all(r[1][22:31] == i64(-2**31) + b"\x00" for r in want)
    rig.drop()


# ------------------------------------------------------------------ churn

def v8(x):
    return i64(x)


def test_retraction_changes_the_frames_of_other_rows(g):
    rig = Rig(g, abi.schema(1, 8), [(0, 8, False)],
              [abi.wf_sum(0, 8, start=P(1), end=F(1)),
               abi.wf_count(start=P(1), end=CUR)])
    rig.push([((9,), v8(x), 0, 1) for x in (1, 2, 3, 4, 5)], 0, 1, "insert")
    # without 3, the rows 2 and 4 are neighbours: their sums change, and
    # nothing else does
    want = rig.push([((9,), v8(3), 1, -1)], 1, 2, "retract the middle")
    assert sorted((r[1][:8], r[3]) for r in want) == sorted(
        [(v8(2), -1), (v8(2), 1), (v8(3), -1), (v8(4), -1), (v8(4), 1)])
    want = rig.push([((9,), v8(7), 2, 1), ((9,), v8(7), 2, -1)], 2, 3,
                    "no net change")
    assert want == []
    # empty the partition, then refill it
    want = rig.push([((9,), v8(x), 3, -1) for x in (1, 2, 4, 5)], 3, 4,
                    "retract the partition")
    assert len(want) == 4 and all(r[3] == -1 for r in want)
    want = rig.push([((9,), v8(x), 4, 2) for x in (6, 7)], 4, 5, "refill")
    assert sum(r[3] for r in want) == 4 and all(r[3] > 0 for r in want)
    rig.drop()


def test_multi_timestamp(g):
    """Two timestamps in one push touch the same partition: corrections at
    both times, the second time's old being the first time's new."""
    rig = Rig(g, abi.schema(1, 8), [(0, 8, True)],
              [abi.wf_sum(0, 8), abi.wf_max(0, 8, start=CUR, end=UF),
               abi.wf_count(start=P(1), end=F(1))])
    rows = [((1,), v8(10), 0, 1), ((1,), v8(30), 0, 2), ((2,), v8(5), 0, 1),
            ((1,), v8(20), 1, 1), ((1,), v8(30), 1, -1), ((3,), v8(6), 1, 1)]
    want = rig.push(rows, 0, 2, "two timestamps")
    assert {r[2] for r in want} == {0, 1}
    at0 = {(r[0], r[1]) for r in want if r[2] == 0 and r[3] > 0}
    assert any((r[0], r[1]) in at0 for r in want if r[2] == 1 and r[3] < 0)
    rig.drop()


def test_aggregates_beside_row_number_and_lag(g):
    rng = np.random.default_rng(17)
    rig = Rig(g, AB, AB_ORDER,
              [abi.wf_row_number(), abi.wf_sum(**X, start=P(2), end=CUR),
               abi.wf_lag(k=1, **X), abi.wf_min(**Y)])
    rows = sized_partition(rng, 1, 300) + sized_partition(rng, 2, 40)
    rig.push(rows, 0, 1, "mixed: load")
    rig.push([(k, v, 1, -1) for k, v, _, m in rows[2:80:7]], 1, 2,
             "mixed: churn")
    rig.drop()


# -------------------------------------------------------- expansion rule

def test_non_expanding_spec_emits_one_row_per_input_row(g):
    """TO_CURRENT / PARTITION / whole-partition ROWS aggregates with RANK
    and LAST_VALUE: one output row per distinct input row, diff = its
    multiplicity — also a multiplicity no expansion could hold."""
    funcs = [abi.wf_count(), abi.wf_min(0, 8, frame=PART), abi.wf_rank(),
             abi.wf_max(0, 8, start=UP, end=UF)]
    assert not any(abi.wf_expands(f) for f in funcs)
    spec = abi.window_spec(abi.schema(1, 8), [(0, 8, False)], funcs)
    op = g.window_create(spec)
    u = abi.make_updates(
        np.array([4, 4, 4], np.int64),
        np.frombuffer(v8(1) + v8(2) + v8(-3), np.uint8),
        np.zeros(3, np.uint64), np.array([2**40, 3, 5], np.int64), 0, 1)
    got = g.window_push(op, u)
    tail = v8(-3) + b"\x00" + i64(6 + 2**40) + v8(2) + b"\x00"
    want = [((4,), v8(-3) + i64(5) + v8(-3) + b"\x00" + i64(1) + v8(2)
             + b"\x00", 0, 5),
            ((4,), v8(1) + i64(5 + 2**40) + v8(-3) + b"\x00" + i64(6)
             + v8(2) + b"\x00", 0, 2**40),
            ((4,), v8(2) + i64(8 + 2**40) + tail, 0, 3)]
    same(got, cols_of(want, 1), "one row per input row")
    g.window_drop(op)


def test_create_refusals_reach_the_c_layer(g):
    from materialize_amd._ffi import MzGpuError
    spec = abi.window_spec(abi.schema(1, 8), [], [abi.wf_min(0, 8)])
    spec.funcs[0].frame = ROWS
    spec.funcs[0].bounds = abi.MZ_WB_PRECEDING | abi.MZ_WB_FOLLOWING << 4
    with pytest.raises(MzGpuError, match="window: func 0: MIN / MAX over a "
                                         "ROWS frame bounded on both sides"):
        g.window_create(spec)
    spec = abi.window_spec(abi.schema(1, 8), [], [abi.wf_sum(0, 8)])
    spec.funcs[0].dflt = 1
    with pytest.raises(MzGpuError, match="an aggregate takes no default"):
        g.window_create(spec)
    spec = abi.window_spec(abi.schema(1, 8), [], [abi.wf_rank()])
    spec.funcs[0].func = 15
    with pytest.raises(MzGpuError, match="unknown func 15"):
        g.window_create(spec)


# ----------------------------------------------------------------- random

def test_random_pushes(g):
    """300 small pushes over 4 keys and a small value universe."""
    rng = np.random.default_rng(23)
    rig = Rig(g, XY, [(9, 4, True)],
              [abi.wf_sum(**FX, start=P(1), end=F(1)), abi.wf_count(**FX),
               abi.wf_min(**FX, start=UP, end=F(1)),
               abi.wf_max(frame=PART, **FY)])
    for t in range(300):
        rows, step = [], {}
        for _ in range(int(rng.integers(1, 4))):
            x = int(rng.integers(-3, 4))
            r = ((int(rng.integers(0, 4)),),
                 xy_row(None if x == 3 else x, int(rng.integers(-2, 2))))
            cur = rig.net.get(r, 0) + step.get(r, 0)
            if cur > 0 and rng.random() < 0.5:
                d = -int(rng.integers(1, cur + 1))
            else:
                d = int(rng.integers(1, 4))
            step[r] = step.get(r, 0) + d
            rows.append((r[0], r[1], t, d))
        rig.push(rows, t, t + 1, f"random push {t}")
    rig.drop()
