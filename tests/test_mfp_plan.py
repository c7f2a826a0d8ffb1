"""Scalar-expression MFP, the parts that need no GPU: the postfix compiler of
abi.mfp_spec, its type and create-time checks, the render surface's refusal
of a context without the operator, and the ctypes mirrors against the C
header's own sizeof / offsetof."""
import os
import shutil
import subprocess

import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, VS = abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_STREAM
IN = abi.schema(1, 16)


def a():
    return abi.x_col(VS, 0)


def b():
    return abi.x_col(VS, 8)


def key_out():
    return abi.x_out_key(abi.x_col(KEY, 0), 0)


def ops_of(sp):
    return [(o.op, o.src, o.width, o.nullable, o.off, o.imm)
            for o in sp.ops[:sp.n_ops]]


def test_fixed_expression_compiles_to_postfix():
    # FILTER a + b > 3; OUT key; OUT IF(b = 0, NULL, a / b) as a nullable i32
    sp = abi.mfp_spec(IN, abi.schema(1, 5), [
        abi.x_filter(a() + b() > 3),
        key_out(),
        abi.x_out_val(abi.x_if(b() == 0, abi.x_null("int"), a() // b()),
                      0, 4, nullable=1)])
    X = abi
    assert ops_of(sp) == [
        (X.MZ_X_COL, VS, 8, 0, 0, 0), (X.MZ_X_COL, VS, 8, 0, 8, 0),
        (X.MZ_X_ADD, 0, 0, 0, 0, 0), (X.MZ_X_LIT, 0, 0, 0, 0, 3),
        (X.MZ_X_GT, 0, 0, 0, 0, 0), (X.MZ_X_FILTER, 0, 0, 0, 0, 0),
        (X.MZ_X_COL, KEY, 8, 0, 0, 0), (X.MZ_X_OUT, 0, 8, 0, 0, 0),
        (X.MZ_X_COL, VS, 8, 0, 8, 0), (X.MZ_X_LIT, 0, 0, 0, 0, 0),
        (X.MZ_X_EQ, 0, 0, 0, 0, 0), (X.MZ_X_NULL, 0, 0, 0, 0, 0),
        (X.MZ_X_COL, VS, 8, 0, 0, 0), (X.MZ_X_COL, VS, 8, 0, 8, 0),
        (X.MZ_X_DIV, 0, 0, 0, 0, 0), (X.MZ_X_IF, 0, 0, 0, 0, 0),
        (X.MZ_X_OUT, 1, 4, 1, 0, 0)]
    assert (sp.in_.key_words, sp.in_.val_bytes) == (1, 16)
    assert (sp.out.key_words, sp.out.val_bytes) == (1, 5)


def test_reflected_and_nary_operators():
    sp = abi.mfp_spec(IN, abi.schema(1, 8), [
        key_out(),
        abi.x_out_val(abi.x_coalesce(a(), b(), 7) + (10 - a()), 0, 8)])
    got = [o[0] for o in ops_of(sp)][2:]
    X = abi
    assert got == [X.MZ_X_COL, X.MZ_X_COL, X.MZ_X_LIT, X.MZ_X_COALESCE,
                   X.MZ_X_COALESCE, X.MZ_X_LIT, X.MZ_X_COL, X.MZ_X_SUB,
                   X.MZ_X_ADD, X.MZ_X_OUT]


def deep_sum(n):
    """c0 + (c1 + (... + c{n-1})): needs a stack of n."""
    e = a()
    for _ in range(n - 1):
        e = a() + e
    return e


def wide_sum(n_ops):
    """((a + a) + a) ..., negated when n_ops is odd: depth 2, and n_ops ops
    with its OUT (k COLs, k - 1 ADDs, the OUT)."""
    e = a()
    for _ in range(n_ops // 2 - 1):
        e = e + a()
    return -e if n_ops % 2 else e


def test_stack_depth_limit():
    out = abi.schema(1, 8)
    abi.mfp_spec(IN, out, [key_out(), abi.x_out_val(deep_sum(8), 0, 8)])
    with pytest.raises(ValueError, match="stack"):
        abi.mfp_spec(IN, out, [key_out(), abi.x_out_val(deep_sum(9), 0, 8)])


def test_program_length_limit():
    out = abi.schema(1, 8)
    # key OUT is 2 ops; 62 more make 64, 63 more make 65
    sp = abi.mfp_spec(IN, out, [key_out(),
                                abi.x_out_val(wide_sum(62), 0, 8)])
    assert sp.n_ops == 64
    with pytest.raises(ValueError, match="65 ops"):
        abi.mfp_spec(IN, out, [key_out(), abi.x_out_val(wide_sum(63), 0, 8)])


BOOL = abi.x_col(VS, 0, width=1)

TYPE_ERRORS = {
    "arith on bool": lambda: BOOL + 1,
    "compare on bool": lambda: BOOL < BOOL,
    "neg on bool": lambda: -BOOL,
    "abs on bool": lambda: abi.x_abs(BOOL),
    "and on int": lambda: a() & b(),
    "or on int": lambda: (a() > 1) | b(),
    "not on int": lambda: ~a(),
    "if cond int": lambda: abi.x_if(a(), 1, 2),
    "if branches": lambda: abi.x_if(a() > 1, a(), BOOL),
    "coalesce types": lambda: abi.x_coalesce(a(), BOOL),
    "null type": lambda: abi.x_null("float"),
    "col width": lambda: abi.x_col(VS, 0, width=2),
    "literal range": lambda: abi.x_lit(2**63),
    "filter on int": lambda: abi.mfp_spec(
        IN, abi.schema(1, 0), [abi.x_filter(a()), key_out()]),
    "width 1 for int": lambda: abi.mfp_spec(
        IN, abi.schema(1, 1), [key_out(), abi.x_out_val(a(), 0, 1)]),
    "width 8 for bool": lambda: abi.mfp_spec(
        IN, abi.schema(1, 8), [key_out(), abi.x_out_val(a() > 1, 0, 8)]),
}


@pytest.mark.parametrize("name", sorted(TYPE_ERRORS))
def test_type_errors(name):
    with pytest.raises(ValueError, match="mfp"):
        TYPE_ERRORS[name]()


def _spec(in_s, out_s, stmts):
    return lambda: abi.mfp_spec(in_s, out_s, stmts)


VALIDATION_ERRORS = {
    "col past val": (_spec(IN, abi.schema(1, 8), [
        key_out(), abi.x_out_val(abi.x_col(VS, 12), 0, 8)]), "reads past"),
    "col null byte past val": (_spec(IN, abi.schema(1, 8), [
        key_out(), abi.x_out_val(abi.x_col(VS, 8, nullable=1), 0, 8)]),
        "reads past"),
    "col past key": (_spec(IN, abi.schema(1, 0), [
        abi.x_out_key(abi.x_col(KEY, 8), 0)]), "reads past"),
    "col bad source": (_spec(IN, abi.schema(1, 0), [
        abi.x_out_key(abi.x_col(abi.MZ_SRC_VAL_LOOKUP, 0), 0)]),
        "MZ_SRC_KEY or MZ_SRC_VAL_STREAM"),
    "out gap in val": (_spec(IN, abi.schema(1, 16), [
        key_out(), abi.x_out_val(a(), 8, 8)]), "gap"),
    "out gap in key": (_spec(IN, abi.schema(2, 0), [key_out()]), "gap"),
    "out overlap": (_spec(IN, abi.schema(1, 12), [
        key_out(), abi.x_out_val(a(), 0, 8), abi.x_out_val(b(), 4, 8)]),
        "overlap"),
    "out null byte overlap": (_spec(IN, abi.schema(1, 16), [
        key_out(), abi.x_out_val(a(), 0, 8, nullable=1),
        abi.x_out_val(b(), 8, 8)]), "overlap"),
    "out past val": (_spec(IN, abi.schema(1, 8), [
        key_out(), abi.x_out_val(a(), 4, 8)]), "writes past"),
    "out bad width": (_spec(IN, abi.schema(1, 2), [
        key_out(), abi.x_out_val(a(), 0, 2)]), "width"),
    "key out nullable": (_spec(IN, abi.schema(1, 0), [
        abi.XStmt(abi.MZ_X_OUT, a(), src=0, off=0, width=8, nullable=1)]),
        "key OUT"),
    "key out width 4": (_spec(IN, abi.schema(1, 0), [
        abi.XStmt(abi.MZ_X_OUT, a(), src=0, off=0, width=4)]), "key OUT"),
    "varlen in": (_spec(abi.schema(1, abi.MZ_GPU_VARLEN), abi.schema(1, 0),
                        [key_out()]), "varlen"),
    "varlen out": (_spec(IN, abi.schema(1, abi.MZ_GPU_VARLEN),
                         [key_out()]), "varlen"),
    "three key words": (_spec(abi.schema(3, 0), abi.schema(1, 0),
                              [key_out()]), "key words"),
    "no key words out": (_spec(IN, abi.schema(0, 0), []), "key words"),
    "wide val": (_spec(abi.schema(1, 72), abi.schema(1, 0), [key_out()]),
                 "64 val bytes"),
}


@pytest.mark.parametrize("name", sorted(VALIDATION_ERRORS))
def test_validation_errors(name):
    fn, msg = VALIDATION_ERRORS[name]
    with pytest.raises(ValueError, match=msg):
        fn()


def test_render_mfp_refuses_the_oracle():
    from pyoracle import OracleCtx
    sp = abi.mfp_spec(IN, abi.schema(1, 0), [key_out()])
    with pytest.raises(NotImplementedError):
        render.render_mfp(OracleCtx(), render.MfpPlan(sp))


LAYOUT_C = r"""
#include <stdio.h>
#include "mz_gpu.h"
int main(void) {
  printf("xop %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mz_gpu_xop),
         offsetof(mz_gpu_xop, op), offsetof(mz_gpu_xop, src),
         offsetof(mz_gpu_xop, width), offsetof(mz_gpu_xop, nullable),
         offsetof(mz_gpu_xop, off), offsetof(mz_gpu_xop, pad),
         offsetof(mz_gpu_xop, imm));
  printf("spec %zu %zu %zu %zu %zu\n", sizeof(mz_gpu_mfp_spec),
         offsetof(mz_gpu_mfp_spec, n_ops), offsetof(mz_gpu_mfp_spec, ops),
         offsetof(mz_gpu_mfp_spec, in), offsetof(mz_gpu_mfp_spec, out));
  printf("consts %d %d %d %d %d %d %d %d\n", MZ_GPU_MAX_XOPS, MZ_GPU_XSTACK,
         MZ_X_COL, MZ_X_OUT, MZ_ERR_INT64_OUT_OF_RANGE,
         MZ_ERR_NUMERIC_FIELD_OVERFLOW, MZ_ERR_INT32_OUT_OF_RANGE,
         MZ_ERR_UNEXPECTED_NULL);
  return 0;
}
"""


def test_ctypes_mirrors_match_the_header(tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True,
                           text=True).stdout.split("\n")
    xop = [int(x) for x in lines[0].split()[1:]]
    spec = [int(x) for x in lines[1].split()[1:]]
    consts = [int(x) for x in lines[2].split()[1:]]
    X, S = abi.XOp, abi.MfpSpec
    assert xop == [abi.C.sizeof(X), X.op.offset, X.src.offset,
                   X.width.offset, X.nullable.offset, X.off.offset,
                   X.pad.offset, X.imm.offset]
    assert xop[0] == 16
    assert spec == [abi.C.sizeof(S), S.n_ops.offset, S.ops.offset,
                    S.in_.offset, S.out.offset]
    assert consts == [abi.MZ_GPU_MAX_XOPS, abi.MZ_GPU_XSTACK, abi.MZ_X_COL,
                      abi.MZ_X_OUT, abi.MZ_ERR_INT64_OUT_OF_RANGE,
                      abi.MZ_ERR_NUMERIC_FIELD_OVERFLOW,
                      abi.MZ_ERR_INT32_OUT_OF_RANGE,
                      abi.MZ_ERR_UNEXPECTED_NULL]
