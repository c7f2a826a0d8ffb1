"""Scalar-expression MFP (mz_gpu_mfp / k_mfp_eval) on the GPU.

Reference: `ev` below, a lazy recursive evaluator over the abi.Expr tree with
Python ints, None for NULL and one exception (EvalErr) per error code. AND /
OR stop at a deciding operand, IF evaluates only the branch it takes,
COALESCE only what it needs. It shares nothing with the postfix compiler of
abi.mfp_spec or with the kernel's eager tagged evaluation. `model` runs the
statements in order over every input row and keeps the passing rows as
(key, val bytes, time) -> wrapping diff sum and the error rows as (code,
time) -> wrapping diff sum.

Every program is run twice: the consolidated output is compared byte for
byte, in the engine's canonical order (keys as signed tuples, vals as
zero-padded little-endian u64 words, then time); the raw output
(consolidate = 0) after consolidating it here. Error rows are compared as
consolidated (code, time, diff) both times. The CPU oracle has no MFP.

A guarded division is not error-free over the whole value pool: the pool has
i64 MIN and -1, and MIN / -1 is MZ_ERR_INT64_OUT_OF_RANGE. So
`IF(b = 0, NULL, a / b)` and `FILTER b <> 0; OUT a / b` over the 8-byte
columns are asserted to have that one error row and no other (no division by
zero); over the 4-byte columns of the same pool (MIN and MAX those of i32)
the quotient always fits and "no error rows at all" is asserted.
"""
import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

pytestmark = pytest.mark.gpu

X = abi
KEY, VS = abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_STREAM
I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1
DIV0, I64OOR, OVERFLOW, I32OOR, UNEXPECTED_NULL = (
    abi.MZ_ERR_DIVISION_BY_ZERO, abi.MZ_ERR_INT64_OUT_OF_RANGE,
    abi.MZ_ERR_NUMERIC_FIELD_OVERFLOW, abi.MZ_ERR_INT32_OUT_OF_RANGE,
    abi.MZ_ERR_UNEXPECTED_NULL)
POOL = [0, 1, -1, 2, -7, I64_MIN, I64_MAX, None]
POOL32 = [0, 1, -1, 2, -7, I32_MIN, I32_MAX, None]


# ------------------------------------------------------------ reference

class EvalErr(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def wrap(d):
    return ((d + 2**63) % 2**64) - 2**63


def val_words(v):
    return tuple(int.from_bytes(v[o:o + 8], "little")
                 for o in range(0, len(v), 8))


def _checked(v):
    if not I64_MIN <= v <= I64_MAX:
        raise EvalErr(OVERFLOW)
    return v


def _arith(op, a, b):
    if op == X.MZ_X_ADD:
        return _checked(a + b)
    if op == X.MZ_X_SUB:
        return _checked(a - b)
    if op == X.MZ_X_MUL:
        return _checked(a * b)
    if b == 0:
        raise EvalErr(DIV0)
    q = abs(a) // abs(b)
    if (a < 0) != (b < 0):
        q = -q
    if op == X.MZ_X_MOD:
        return a - q * b  # the sign follows the dividend
    if q > I64_MAX:
        raise EvalErr(I64OOR)
    return q


_CMP = {X.MZ_X_LT: lambda a, b: a < b, X.MZ_X_LE: lambda a, b: a <= b,
        X.MZ_X_GT: lambda a, b: a > b, X.MZ_X_GE: lambda a, b: a >= b,
        X.MZ_X_EQ: lambda a, b: a == b, X.MZ_X_NE: lambda a, b: a != b}


def ev(e, key, val):
    """The value of `e` over the row (key bytes, val bytes): an int (bools
    as 0 / 1), None for NULL; raises EvalErr."""
    op = e.op
    if op == X.MZ_X_COL:
        src = key if e.src == KEY else val
        if e.nullable and src[e.off + e.width] != 0:
            return None
        if e.width == 1:
            return int(src[e.off] != 0)
        return int.from_bytes(src[e.off:e.off + e.width], "little",
                              signed=True)
    if op == X.MZ_X_LIT:
        return e.imm
    if op == X.MZ_X_NULL:
        return None
    if op == X.MZ_X_IS_NULL:
        return int(ev(e.args[0], key, val) is None)
    if op in (X.MZ_X_NEG, X.MZ_X_ABS, X.MZ_X_NOT):
        a = ev(e.args[0], key, val)
        if a is None:
            return None
        if op == X.MZ_X_NOT:
            return int(not a)
        if a == I64_MIN:
            raise EvalErr(I64OOR)
        return -a if op == X.MZ_X_NEG else abs(a)
    if op in (X.MZ_X_AND, X.MZ_X_OR):
        decides = int(op == X.MZ_X_OR)
        err, null = None, False
        for arg in e.args:
            try:
                a = ev(arg, key, val)
            except EvalErr as ex:
                err = err or ex  # the left one first
                continue
            if a is None:
                null = True
            elif a == decides:
                return decides  # the operands after it are not looked at
        if err:
            raise err
        return None if null else 1 - decides
    if op == X.MZ_X_IF:
        c = ev(e.args[0], key, val)
        return ev(e.args[1] if c else e.args[2], key, val)
    if op == X.MZ_X_COALESCE:
        a = ev(e.args[0], key, val)
        return a if a is not None else ev(e.args[1], key, val)
    a = ev(e.args[0], key, val)
    b = ev(e.args[1], key, val)  # evaluated before the NULL check
    if a is None or b is None:
        return None
    if op in _CMP:
        return int(_CMP[op](a, b))
    return _arith(op, a, b)


def run_row(stmts, okw, ovb, key, val):
    """("ok", out key tuple, out val bytes) | ("drop",) | ("err", code)."""
    okey, oval = bytearray(8 * okw), bytearray(ovb)
    for st in stmts:
        try:
            v = ev(st.expr, key, val)
        except EvalErr as ex:
            return ("err", ex.code)
        if st.op == X.MZ_X_FILTER:
            if not v:
                return ("drop",)
            continue
        if v is None and not st.nullable:
            return ("err", UNEXPECTED_NULL)
        if v is not None and st.width == 4 and not I32_MIN <= v <= I32_MAX:
            return ("err", I32OOR)
        dst = okey if st.src == 0 else oval
        dst[st.off:st.off + st.width] = (v or 0).to_bytes(
            st.width, "little", signed=True)
        if st.nullable:
            dst[st.off + st.width] = int(v is None)
    return ("ok", tuple(int.from_bytes(okey[o:o + 8], "little", signed=True)
                        for o in range(0, 8 * okw, 8)), bytes(oval))


def cols_of(rows, errs):
    rows = sorted(((k, v, t, d) for (k, v, t), d in rows.items() if d),
                  key=lambda r: (r[0], val_words(r[1]), r[2]))
    e = sorted((c, t, d) for (c, t), d in errs.items() if d)
    return ((np.array([x for r in rows for x in r[0]], np.int64),
             np.frombuffer(b"".join(r[1] for r in rows), np.uint8),
             np.array([r[2] for r in rows], np.uint64),
             np.array([r[3] for r in rows], np.int64)),
            (np.array([x[0] for x in e], np.uint64),
             np.array([x[1] for x in e], np.uint64),
             np.array([x[2] for x in e], np.int64)))


def model(stmts, kw, okw, ovb, keys, vals, times, diffs):
    """-> (ok columns, error columns, per-row results)."""
    rows, errs, res = {}, {}, []
    for i in range(len(times)):
        key = np.ascontiguousarray(keys[i * kw:(i + 1) * kw],
                                   np.int64).tobytes()
        r = run_row(stmts, okw, ovb, key, vals[i].tobytes())
        res.append(r)
        t, d = int(times[i]), int(diffs[i])
        if r[0] == "ok":
            k = (r[1], r[2], t)
            rows[k] = wrap(rows.get(k, 0) + d)
        elif r[0] == "err":
            errs[(r[1], t)] = wrap(errs.get((r[1], t), 0) + d)
    return cols_of(rows, errs) + (res,)


def host_consolidate(cols, okw, ovb):
    k, v, t, d = cols
    rows = {}
    v = np.asarray(v).reshape(len(t), ovb)
    for i in range(len(t)):
        key = (tuple(int(x) for x in k[i * okw:(i + 1) * okw]),
               v[i].tobytes(), int(t[i]))
        rows[key] = wrap(rows.get(key, 0) + int(d[i]))
    return cols_of(rows, {})[0]


def same(got, want, what, cols=("keys", "vals", "times", "diffs")):
    for a, b, col in zip(got, want, cols):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype.itemsize == b.dtype.itemsize, f"{what}: {col} dtype"
        np.testing.assert_array_equal(
            np.ascontiguousarray(a).view(np.uint8),
            np.ascontiguousarray(b).view(np.uint8), err_msg=f"{what}: {col}")


ERR_COLS = ("err codes", "err times", "err diffs")


def check(g, in_s, out_s, stmts, keys, vals, times, diffs, what):
    """Run the program both ways against the model; -> the per-row results
    of the model."""
    spec = abi.mfp_spec(in_s, out_s, stmts)
    kw, okw, ovb = in_s.key_words, out_s.key_words, out_s.val_bytes
    keys = np.ascontiguousarray(keys, np.int64).ravel()
    vals = np.ascontiguousarray(vals, np.uint8).reshape(len(times),
                                                        in_s.val_bytes)
    want, want_errs, res = model(stmts, kw, okw, ovb, keys, vals, times,
                                 diffs)
    lo, hi = 0, int(max(times, default=0)) + 1
    u = abi.make_updates(keys, vals.ravel() if in_s.val_bytes else None,
                         times, diffs, lo, hi)
    got = g.mfp(spec, u)
    same(got, want, f"{what}: consolidated")
    same(g.last_errs, want_errs, f"{what}: consolidated", ERR_COLS)
    raw = g.mfp(spec, u, consolidate=False)
    assert len(raw[2]) == sum(r[0] == "ok" for r in res), f"{what}: raw n"
    same(host_consolidate(raw, okw, ovb), want, f"{what}: raw")
    same(g.last_errs, want_errs, f"{what}: raw", ERR_COLS)
    return res


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


# ---------------------------------------------------------------- inputs
# The input row of the directed and fuzz cases: 2 key words and
#   a  i64 @0  null @8     b  i64 @9  null @17
#   a4 i32 @18 null @22    b4 i32 @23 null @27    f bool @28 null @29
IN = abi.schema(2, 30)
A = abi.x_col(VS, 0, 8, 1)
B = abi.x_col(VS, 9, 8, 1)
A4 = abi.x_col(VS, 18, 4, 1)
B4 = abi.x_col(VS, 23, 4, 1)
F = abi.x_col(VS, 28, 1, 1)
K0 = abi.x_col(KEY, 0)
K1 = abi.x_col(KEY, 8)


def pack_rows(avals, bvals, a4vals, b4vals, fvals):
    n = len(avals)
    v = np.zeros((n, 30), np.uint8)
    for i in range(n):
        for off, w, x in ((0, 8, avals[i]), (9, 8, bvals[i]),
                          (18, 4, a4vals[i]), (23, 4, b4vals[i]),
                          (28, 1, fvals[i])):
            if x is None:
                v[i, off + w] = 1
                # garbage under a NULL: the null byte alone decides
                v[i, off:off + w] = 0xA5 if w > 1 else 1
            else:
                v[i, off:off + w] = np.frombuffer(
                    int(x).to_bytes(w, "little", signed=True), np.uint8)
    return v


def cross_rows():
    """The 64 rows of POOL x POOL in (a, b), POOL32 x POOL32 in (a4, b4)."""
    ia = [i for i in range(8) for _ in range(8)]
    ib = [j for _ in range(8) for j in range(8)]
    vals = pack_rows([POOL[i] for i in ia], [POOL[j] for j in ib],
                     [POOL32[i] for i in ia], [POOL32[j] for j in ib],
                     [(1, 0, None)[(i + j) % 3] for i, j in zip(ia, ib)])
    keys = np.array([[i, 7] for i in range(64)], np.int64)
    times = np.arange(64, dtype=np.uint64) % 3
    diffs = np.array([(1, -1, 2, -2)[i % 4] for i in range(64)], np.int64)
    return keys, vals, times, diffs, ia, ib


KEYS_OUT = [abi.x_out_key(K0, 0), abi.x_out_key(K1, 8)]


def out8(e, off=0):
    return abi.x_out_val(e, off, 8, nullable=1)


def directed_programs():
    """name -> (out val bytes, statements)."""
    p = {}
    for name, e in (("add", A + B), ("sub", A - B), ("mul", A * B),
                    ("div", A // B), ("mod", A % B), ("neg", -A),
                    ("abs", abi.x_abs(B))):
        p[name] = (9, KEYS_OUT + [out8(e)])
    p["compare"] = (12, KEYS_OUT + [
        abi.x_out_val(e, 2 * i, 1, nullable=1) for i, e in enumerate(
            (A < B, A <= B, A > B, A >= B, A == B, A != B))])
    p["not is_null"] = (4, KEYS_OUT + [
        abi.x_out_val(~(A < B), 0, 1, nullable=1),
        abi.x_out_val(abi.x_is_null(A), 2, 1),
        abi.x_out_val(abi.x_is_null(F), 3, 1)])
    p["is_null of error"] = (1, KEYS_OUT + [
        abi.x_out_val(abi.x_is_null(A // B), 0, 1)])
    p["and"] = (2, KEYS_OUT + [
        abi.x_out_val((A != 0) & (A // B > 0), 0, 1, nullable=1)])
    p["or"] = (2, KEYS_OUT + [
        abi.x_out_val((A == 0) | (A // B > 0), 0, 1, nullable=1)])
    p["and or of bools"] = (4, KEYS_OUT + [
        abi.x_out_val(F & (A < B), 0, 1, nullable=1),
        abi.x_out_val(F | (A < B), 2, 1, nullable=1)])
    p["and error left"] = (2, KEYS_OUT + [
        abi.x_out_val((A // B > 0) & (B + B > 0), 0, 1, nullable=1)])
    p["if"] = (9, KEYS_OUT + [
        out8(abi.x_if(B == 0, abi.x_null("int"), A // B))])
    p["if 32"] = (9, KEYS_OUT + [
        out8(abi.x_if(B4 == 0, abi.x_null("int"), A4 // B4))])
    p["if null cond"] = (9, KEYS_OUT + [out8(abi.x_if(F, A, B))])
    p["coalesce"] = (8, KEYS_OUT + [
        abi.x_out_val(abi.x_coalesce(A, B, 0) * 2, 0, 8)])
    p["store i32"] = (5, KEYS_OUT + [
        abi.x_out_val(abi.x_coalesce(A, 3) + abi.x_coalesce(B, 4), 0, 4,
                      nullable=1)])
    p["unexpected null"] = (8, KEYS_OUT + [abi.x_out_val(A, 0, 8)])
    p["sign extension"] = (27, KEYS_OUT + [
        out8(A4, 0), out8(A4 + B4, 9), out8(A4 * B4, 18)])
    p["filter"] = (0, KEYS_OUT + [abi.x_filter(A // B > 0)])
    p["filter bool col"] = (0, [abi.x_filter(~F)] + KEYS_OUT)
    return p


# ----------------------------------------------------------------- cases

def test_directed_table(g):
    keys, vals, times, diffs, ia, ib = cross_rows()
    seen = set()
    results = {}
    for name, (ovb, stmts) in directed_programs().items():
        res = check(g, IN, abi.schema(2, ovb), stmts, keys, vals, times,
                    diffs, name)
        results[name] = res
        seen |= {r[1] for r in res if r[0] == "err"}
    assert seen >= {DIV0, I64OOR, OVERFLOW, I32OOR, UNEXPECTED_NULL}
    row = {(POOL[i], POOL[j]): n for n, (i, j) in enumerate(zip(ia, ib))}
    # false AND error -> false; true OR error -> true (a = 0, b = 0)
    assert results["and"][row[0, 0]][2] == bytes([0, 0])
    assert results["or"][row[0, 0]][2] == bytes([1, 0])
    # ... and the unmasked error is there (a = 1, b = 0)
    assert results["and"][row[1, 0]] == ("err", DIV0)
    assert results["or"][row[1, 0]] == ("err", DIV0)
    # an error on the right beats a NULL on the left
    assert results["div"][row[1, 0]] == ("err", DIV0)
    assert results["div"][row[None, 0]][0] == "ok"
    assert results["add"][row[I64_MAX, 1]] == ("err", OVERFLOW)
    assert results["mod"][row[I64_MIN, -1]][2] == bytes(9)
    # the guard masks every division by zero; over the 8-byte columns
    # MIN / -1 is left, over the 4-byte ones nothing is
    assert [r for r in results["if"] if r[0] == "err"] == [("err", I64OOR)]
    assert results["if"][row[I64_MIN, -1]] == ("err", I64OOR)
    assert all(r[0] == "ok" for r in results["if 32"])
    # 4-byte columns sign-extend: -7 and i32 MIN come out as i64
    sx = results["sign extension"][row[-7, I64_MIN]][2]
    assert int.from_bytes(sx[0:8], "little", signed=True) == -7
    assert int.from_bytes(sx[9:17], "little", signed=True) == -7 + I32_MIN
    assert int.from_bytes(sx[18:26], "little", signed=True) == -7 * I32_MIN


def test_statement_order(g):
    keys, vals, times, diffs, ia, ib = cross_rows()
    for a, b, name in ((A4, B4, "32"), (A, B, "64")):
        first = [abi.x_filter(b != 0)] + KEYS_OUT + [out8(a // b)]
        late = KEYS_OUT + [out8(a // b), abi.x_filter(b != 0)]
        r1 = check(g, IN, abi.schema(2, 9), first, keys, vals, times, diffs,
                   f"filter first {name}")
        r2 = check(g, IN, abi.schema(2, 9), late, keys, vals, times, diffs,
                   f"filter last {name}")
        e1 = [r for r in r1 if r[0] == "err"]
        assert e1 == ([] if name == "32" else [("err", I64OOR)])
        pool = POOL32 if name == "32" else POOL
        for n, (i, j) in enumerate(zip(ia, ib)):
            if pool[j] == 0 and pool[i] is not None:
                assert r1[n] == ("drop",) and r2[n] == ("err", DIV0)
            else:
                assert r1[n] == r2[n]


def raw_spec(in_s, out_s, ops):
    """An MfpSpec put together by hand, past the builder's checks."""
    sp = abi.MfpSpec()
    sp.n_ops = len(ops)
    for i, o in enumerate(ops[:abi.MZ_GPU_MAX_XOPS]):
        sp.ops[i] = o
    sp.in_, sp.out = in_s, out_s
    return sp


def test_c_layer_refuses(g):
    """mz_gpu_mfp validates on its own: programs the Python builder would
    never emit fail the call with a message and launch nothing."""
    from materialize_amd._ffi import MzGpuError
    O = abi.XOp
    col = O(op=X.MZ_X_COL, src=VS, width=8, off=0)
    okey = O(op=X.MZ_X_OUT, src=0, width=8, off=0)
    s10, s18 = abi.schema(1, 0), abi.schema(1, 8)
    bad = {
        "underflow": (s18, s10, [O(op=X.MZ_X_ADD), okey], "underflow"),
        "left on the stack": (s18, s10, [col, col, okey], "not empty"),
        "not empty at the end": (s18, s10, [col, okey, col], "not empty"),
        "too deep": (s18, s10, [col] * 9 + [O(op=X.MZ_X_ADD)] * 8 + [okey],
                     "deeper"),
        "too long": (s18, s10, [col, okey] * 33, "n_ops"),
        "unknown opcode": (s18, s10, [O(op=77), okey], "unknown opcode"),
        "col past the val": (s18, s10, [O(op=X.MZ_X_COL, src=VS, width=8,
                                          off=1), okey], "reads past"),
        "col from the lookup side": (s18, s10, [O(
            op=X.MZ_X_COL, src=abi.MZ_SRC_VAL_LOOKUP, width=8), okey],
            "MZ_SRC_KEY"),
        "gap": (s18, s18, [col, okey], "gap"),
        "overlap": (s18, s10, [col, okey, col, okey], "overlap"),
        "out past the key": (s18, s10, [col, O(op=X.MZ_X_OUT, src=0, width=8,
                                               off=8)], "writes past"),
        "nullable key": (s18, abi.schema(2, 0), [col, O(
            op=X.MZ_X_OUT, src=0, width=8, nullable=1)], "key OUT"),
        "varlen": (abi.schema(1, abi.MZ_GPU_VARLEN), s10, [okey], "varlen"),
        "three key words": (abi.schema(3, 0), s10, [col, okey], "key words"),
    }
    u = abi.make_updates(np.array([1], np.int64), np.zeros(8, np.uint8),
                         np.zeros(1, np.uint64), np.ones(1, np.int64), 0, 1)
    for name, (in_s, out_s, ops, msg) in bad.items():
        with pytest.raises(MzGpuError, match=msg):
            g.mfp(raw_spec(in_s, out_s, ops), u)
    # ... and the context is as good as before
    k, v, t, d = g.mfp(raw_spec(s18, s18, [col, okey, col, O(
        op=X.MZ_X_OUT, src=1, width=8)]), u)
    assert (k.tolist(), v.view(np.int64).tolist(), d.tolist()) == \
        ([0], [0], [1])


def random_rows(rng, n, nkeys=5):
    pick = lambda pool: [pool[i] for i in rng.integers(0, 8, n)]
    vals = pack_rows(pick(POOL), pick(POOL), pick(POOL32), pick(POOL32),
                     [(1, 0, None)[i] for i in rng.integers(0, 3, n)])
    keys = np.stack([np.array([POOL[i] for i in rng.integers(0, 7, n)],
                              np.int64),
                     rng.integers(0, nkeys, n)], axis=1).astype(np.int64)
    times = rng.integers(0, 3, n).astype(np.uint64)
    diffs = rng.choice([-2, -1, 1, 2], n).astype(np.int64)
    return keys, vals, times, diffs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_tails(g, n):
    rng = np.random.default_rng(1000 + n)
    keys, vals, times, diffs = random_rows(rng, n)
    stmts = [abi.x_filter(abi.x_coalesce(A4 < B4, F, True)),
             abi.x_out_key(K1 + 1, 0),
             out8(abi.x_if(B == 0, abi.x_null("int"), A4 // B), 0),
             abi.x_out_val(abi.x_coalesce(A4, -1), 9, 4)]
    res = check(g, IN, abi.schema(1, 13), stmts, keys, vals, times, diffs,
                f"n={n}")
    assert len(res) == n
    if n == 0:
        spec = abi.mfp_spec(IN, abi.schema(1, 13), stmts)
        u = abi.make_updates(np.empty(0, np.int64), None,
                             np.empty(0, np.uint64), np.empty(0, np.int64),
                             0, 1)
        for cons in (True, False):
            out = g.mfp(spec, u, consolidate=cons)
            assert [len(c) for c in out] == [0, 0, 0, 0]
            assert [len(c) for c in g.last_errs] == [0, 0, 0]


# ------------------------------------------------------------------ fuzz

INT_COLS = (A, B, A4, B4, K0, K1)
ARITH = ("__add__", "__sub__", "__mul__", "__floordiv__", "__mod__")
CMPS = ("__lt__", "__le__", "__gt__", "__ge__", "__eq__", "__ne__")


def gen(rng, typ, depth):
    """A random expression of type `typ`, at most `depth` operators deep."""
    if depth == 0 or rng.random() < 0.3:
        r = rng.random()
        if typ == "int":
            if r < 0.7:
                return INT_COLS[rng.integers(len(INT_COLS))]
            if r < 0.95:
                return abi.x_lit(POOL[rng.integers(7)])
            return abi.x_null("int")
        if r < 0.6:
            return F
        if r < 0.9:
            return abi.x_lit(bool(rng.integers(2)))
        return abi.x_null("bool")
    d = depth - 1
    k = rng.integers(10)
    if k == 8:
        return abi.x_if(gen(rng, "bool", d), gen(rng, typ, d),
                        gen(rng, typ, d))
    if k == 9:
        return abi.x_coalesce(gen(rng, typ, d), gen(rng, typ, d))
    if typ == "int":
        if k == 6:
            return -gen(rng, "int", d)
        if k == 7:
            return abi.x_abs(gen(rng, "int", d))
        return getattr(gen(rng, "int", d), ARITH[rng.integers(5)])(
            gen(rng, "int", d))
    if k == 4:
        return gen(rng, "bool", d) & gen(rng, "bool", d)
    if k == 5:
        return gen(rng, "bool", d) | gen(rng, "bool", d)
    if k == 6:
        return ~gen(rng, "bool", d)
    if k == 7:
        return abi.x_is_null(gen(rng, ("int", "bool")[rng.integers(2)], d))
    return getattr(gen(rng, "int", d), CMPS[rng.integers(6)])(
        gen(rng, "int", d))


def gen_program(rng):
    """-> (out schema, statements): 1-2 filters and OUTs that tile a random
    out schema, in a random statement order."""
    okw = int(rng.integers(1, 3))
    stmts = [abi.x_filter(gen(rng, "bool", 3))
             for _ in range(rng.integers(1, 3))]
    for w in range(okw):
        # a key is mostly a plain column; an expression may be NULL
        e = (K0, K1)[rng.integers(2)] if rng.random() < 0.6 \
            else abi.x_coalesce(gen(rng, "int", 2), 11)
        stmts.append(abi.x_out_key(e, 8 * w))
    off = 0
    for _ in range(rng.integers(0, 4)):
        width = (1, 4, 8)[rng.integers(3)]
        nullable = int(rng.random() < 0.6)
        if width == 4 and rng.random() < 0.7:
            # mostly in range, so that not every row errors
            e = gen(rng, "int", 2) % 1000
        else:
            e = gen(rng, "bool" if width == 1 else "int", 3)
        stmts.append(abi.x_out_val(e, off, width, nullable))
        off += width + nullable
    order = rng.permutation(len(stmts))
    return abi.schema(okw, off), [stmts[i] for i in order]


FUZZ_SEED = 20
FUZZ_PROGRAMS = 40


def fuzz_cases():
    """The 40 programs with their rows, and the number of draws the builder
    rejected."""
    rng = np.random.default_rng(FUZZ_SEED)
    cases, rejected = [], 0
    while len(cases) < FUZZ_PROGRAMS:
        out_s, stmts = gen_program(rng)
        try:
            abi.mfp_spec(IN, out_s, stmts)
        except ValueError as ex:
            assert "stack" in str(ex) or "ops" in str(ex), ex
            rejected += 1
            continue
        keys, vals, times, diffs = random_rows(rng, 700)
        # a pair whose diffs wrap when summed
        keys[1], vals[1], times[1] = keys[0], vals[0], times[0]
        diffs[0], diffs[1] = I64_MAX, 2
        cases.append((out_s, stmts, keys, vals, times, diffs))
    return cases, rejected


def test_fuzz(g):
    cases, rejected = fuzz_cases()
    assert rejected <= 0.05 * (len(cases) + rejected)
    count = {"ok": 0, "drop": 0, "err": 0}
    for i, (out_s, stmts, keys, vals, times, diffs) in enumerate(cases):
        for r in check(g, IN, out_s, stmts, keys, vals, times, diffs,
                       f"fuzz program {i}"):
            count[r[0]] += 1
    total = sum(count.values())
    assert total == 700 * FUZZ_PROGRAMS
    # on the reference alone: the fuzz reaches every class of row
    assert min(count.values()) >= 0.05 * total, count


def test_full_width(g):
    """In and out both 2 key words and 64 val bytes."""
    sch = abi.schema(2, 64)
    rng = np.random.default_rng(5)
    n = 300
    keys = rng.integers(-4, 4, (n, 2)).astype(np.int64)
    v = rng.integers(-50, 50, (n, 8)).astype(np.int64)
    v[rng.random((n, 8)) < 0.05] = I64_MAX
    v[rng.random((n, 8)) < 0.05] = I64_MIN
    c = [abi.x_col(VS, 8 * i) for i in range(8)]
    stmts = [abi.x_out_key(K1, 0), abi.x_out_key(K0 + c[7], 8),
             abi.x_filter(c[0] + c[1] > c[2])]
    stmts += [abi.x_out_val(c[7 - i], 8 * i, 8) for i in range(6)]
    stmts += [abi.x_out_val(c[0] * c[1], 48, 8),
              abi.x_out_val(abi.x_if(c[3] == 0, 0, c[2] % c[3]), 56, 8)]
    check(g, sch, sch, stmts, keys, v.view(np.uint8),
          rng.integers(0, 3, n).astype(np.uint64),
          rng.choice([-1, 1], n).astype(np.int64), "full width")


def np_consolidate(packed, diffs):
    """The distinct values of an int64 array with their wrapping diff sums,
    zeros dropped, ascending."""
    uniq, inv = np.unique(packed, return_inverse=True)
    s = np.zeros(len(uniq), np.int64)
    np.add.at(s, inv.ravel(), diffs)
    return uniq[s != 0], s[s != 0]


# The kernel's grid is capped at 2048 blocks of 256 threads; a thread takes
# 8 rows per iteration. The first size is the cap times the block size plus
# a ragged tail: the threads' row loop, its last turn partly idle. The second
# is 8 times that, where every thread also runs a second, mostly idle
# iteration of the grid-stride loop.
@pytest.mark.parametrize("n", [2048 * 256 + 77, 2048 * 256 * 8 + 77])
def test_grid_stride(g, n):
    """FILTER a < c; OUT key; OUT a / b; OUT a + b with b in [0, 7], against
    a vectorised numpy reference. Keys are below 2^20 and both out fields
    below 2^10, so (key, a / b, a + b, time) packs into one i64 whose order
    is the canonical order of the rows."""
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 1 << 20, n).astype(np.int64)
    a = rng.integers(0, 1000, n).astype(np.int64)
    b = rng.integers(0, 8, n).astype(np.int64)
    c = rng.integers(0, 1000, n).astype(np.int64)
    times = rng.integers(0, 3, n).astype(np.uint64)
    diffs = rng.choice([-1, 1], n).astype(np.int64)
    ca, cb, cc = (abi.x_col(VS, 8 * i) for i in range(3))
    in_s, out_s = abi.schema(1, 24), abi.schema(1, 16)
    spec = abi.mfp_spec(in_s, out_s, [
        abi.x_filter(ca < cc), abi.x_out_key(K0, 0),
        abi.x_out_val(ca // cb, 0, 8), abi.x_out_val(ca + cb, 8, 8)])
    u = abi.make_updates(keys, np.stack([a, b, c], 1).view(np.uint8), times,
                         diffs, 0, 3)

    def pack(k, v0, v1, t):
        assert v0.max() < 1 << 10 and v1.max() < 1 << 10
        return (((k << 10 | v0) << 10 | v1) << 2) | t

    def pack_cols(cols):
        k, v, t, d = cols
        v = np.asarray(v).view(np.int64).reshape(len(d), 2)
        return pack(k, v[:, 0], v[:, 1], np.asarray(t).astype(np.int64)), d

    keep = a < c
    ok, bad = keep & (b != 0), keep & (b == 0)
    t = times.astype(np.int64)
    want, wd = np_consolidate(
        pack(keys[ok], a[ok] // np.maximum(b[ok], 1), a[ok] + b[ok], t[ok]),
        diffs[ok])
    et, ed = np_consolidate(t[bad], diffs[bad])
    assert len(wd) > n // 4 and len(ed) == 3

    def errs_ok():
        gc, gt, gd = g.last_errs
        assert (gc == DIV0).all()
        np.testing.assert_array_equal(gt.astype(np.int64), et)
        np.testing.assert_array_equal(gd, ed)

    got, gd = pack_cols(g.mfp(spec, u))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(gd, wd)
    errs_ok()
    raw = g.mfp(spec, u, consolidate=False)
    assert len(raw[2]) == ok.sum()
    rp, rd = np_consolidate(*pack_cols(raw))
    np.testing.assert_array_equal(rp, want)
    np.testing.assert_array_equal(rd, wd)
    errs_ok()


def test_against_map(g):
    """tests/test_map.py's scenario (filter val[0] > 10; re-key to val[1];
    out val = (old key, val[0])) as an MFP program: the same consolidated
    rows as mz_gpu_map's output, consolidated."""
    rng = np.random.default_rng(55)
    n = 3000
    keys = rng.integers(-100, 100, n).astype(np.int64)
    vals = rng.integers(0, 50, (n, 2)).astype(np.int64)
    diffs = rng.choice([-2, -1, 1, 2], n).astype(np.int64)
    sch = abi.schema(1, 16)
    u = abi.make_updates(keys, vals.view(np.uint8),
                         np.arange(n, dtype=np.uint64) % 3, diffs, 0, 3)
    cl = abi.closure(
        [abi.filt(VS, 0, 8, abi.MZ_CMP_GT, 10)], [abi.field(VS, 8, 8)],
        [abi.field(KEY, 0, 8), abi.field(VS, 0, 8)], sch)
    mk, mv, mt, md = g.map(sch, u, cl)
    assert len(mt) == (vals[:, 0] > 10).sum()
    want = g.consolidate(sch, abi.make_updates(mk, mv, mt, md, 0, 3))
    v0, v1 = abi.x_col(VS, 0), abi.x_col(VS, 8)
    spec = abi.mfp_spec(sch, sch, [
        abi.x_filter(v0 > 10), abi.x_out_key(v1, 0),
        abi.x_out_val(K0, 0, 8), abi.x_out_val(v0, 8, 8)])
    same(g.mfp(spec, u), want, "mfp against map")
    assert len(g.last_errs[0]) == 0
    raw = g.mfp(spec, u, consolidate=False)
    same(g.consolidate(sch, abi.make_updates(*raw, 0, 3)), want,
         "raw mfp against map")


def test_temporal_mfp_reduce(g):
    """render_temporal_filter -> render_mfp (a division by a sometimes-zero
    field, raw output) -> render_reduce (COUNT, SUM): 3 pushes of 200 rows.
    After every push the accumulated reduce output equals the CPU oracle's
    reduce over a from-scratch recompute of the quotients of the rows whose
    window contains now = upper - 1, and the MFP's error rows are the
    divisions by zero among the updates the temporal filter released, at the
    times it gave them."""
    from pyoracle import OracleCtx
    W = 3
    sch = abi.schema(1, 24)  # val: ts, a, b
    out_s = abi.schema(1, 8)
    bounds = [abi.time_bound(abi.MZ_CMP_GE, VS, 0),
              abi.time_bound(abi.MZ_CMP_LT, VS, 0, add=W)]
    tf = render.render_temporal_filter(
        g, render.TemporalFilterPlan(abi.temporal_spec(sch, bounds)))
    mfp = render.render_mfp(g, render.MfpPlan(abi.mfp_spec(sch, out_s, [
        abi.x_out_key(K0, 0),
        abi.x_out_val(abi.x_col(VS, 8) // abi.x_col(VS, 16), 0, 8)]),
        consolidate=False))
    aggs = [abi.Aggregate(func=abi.MZ_AGG_COUNT, off=0, width=8),
            abi.Aggregate(func=abi.MZ_AGG_SUM_I64, off=0, width=8)]
    rspec = abi.reduce_spec(aggs, out_s)
    red = render.render_reduce(g, render.ReducePlan(rspec))
    rng = np.random.default_rng(11)
    inputs = []  # (key, ts, a, b, t, d)
    alive = []
    acc = {}
    saw_errs = 0
    for lower, upper in ((0, 2), (2, 4), (4, 7)):
        new, fresh = [], []
        for _ in range(200):
            t = int(rng.integers(lower, upper))
            if alive and rng.random() < 0.3:
                new.append(alive.pop(int(rng.integers(len(alive)))) + (t, -1))
            else:
                row = (int(rng.integers(8)), t + int(rng.integers(0, 3)),
                       int(rng.integers(-100, 100)), int(rng.integers(0, 4)))
                fresh.append(row)
                new.append(row + (t, 1))
        inputs += new
        alive += fresh
        arr = np.array(new, np.int64)
        tout = tf.push(abi.make_updates(
            arr[:, 0].copy(), arr[:, 1:4].copy().view(np.uint8),
            arr[:, 4].astype(np.uint64), arr[:, 5].copy(), lower, upper))
        mout = mfp.push(tout.updates(lower, upper))
        assert not mout.sorted
        # the error rows: released updates with b = 0
        want_errs = {}
        for key, ts, a, b, t, d in inputs:
            lo, hi = max(t, ts), ts + W
            if b == 0 and hi > lo:
                for time, diff in ((lo, d), (hi, -d)):
                    if lower <= time < upper:
                        want_errs[time] = want_errs.get(time, 0) + diff
        want_errs = sorted((t, d) for t, d in want_errs.items() if d)
        ec, et, ed = mout.errs_to_host()
        assert (ec == DIV0).all()
        assert list(zip(et.tolist(), ed.tolist())) == want_errs
        saw_errs += len(want_errs)
        if mout.n:
            ro = red.push(mout.updates(lower, upper))
            rk, rv, _, rd = ro.to_host()
            ro.release()
            rv = rv.reshape(len(rd), -1)
            for j in range(len(rd)):
                key = (int(rk[j]), rv[j].tobytes())
                acc[key] = acc.get(key, 0) + int(rd[j])
        mout.release()
        tout.release()
        now = upper - 1
        live = {}
        for key, ts, a, b, t, d in inputs:
            if max(t, ts) <= now < ts + W and b != 0:
                q = abs(a) // b * (1 if a >= 0 else -1)
                live[(key, q)] = live.get((key, q), 0) + d
        rows = sorted(r for r, m in live.items() if m)
        o = OracleCtx()
        wk, wv, _, wd = o.reduce_push(o.reduce_create(rspec),
                                      abi.make_updates(
            np.array([r[0] for r in rows], np.int64),
            np.array([r[1] for r in rows], np.int64).view(np.uint8),
            np.zeros(len(rows), np.uint64),
            np.array([live[r] for r in rows], np.int64), 0, 1))
        wv = np.asarray(wv).reshape(len(wd), -1)
        want = {(int(wk[j]), wv[j].tobytes()): int(wd[j])
                for j in range(len(wd))}
        o.close()
        assert {r: m for r, m in acc.items() if m} == want, \
            f"reduce after [{lower}, {upper})"
    assert saw_errs
    tf.drop()
    red.drop()
