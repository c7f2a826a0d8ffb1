"""Window functions, the parts that need no GPU: abi.window_spec's derived
out schema and function layout, its create-time checks, the render
surface's refusal of a context without the operator, and the ctypes mirrors
against the C header's own sizeof / offsetof."""
import os
import shutil
import subprocess

import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN = abi.schema(1, 17)  # a i32 @0, b i32 @4, x i64 @8 with null byte @16
ORDER = [(0, 4, True), (4, 4, False)]
PART = abi.MZ_WF_FRAME_PARTITION


def test_window_spec_derives_out_and_lays_out_funcs():
    funcs = [abi.wf_row_number(),
             abi.wf_lag(8, 8, 2, nullable=1, default=-5),
             abi.wf_dense_rank(),
             abi.wf_last_value(0, 4, frame=PART)]
    sp = abi.window_spec(IN, ORDER, funcs)
    assert (sp.in_.key_words, sp.in_.val_bytes) == (1, 17)
    assert (sp.out.key_words, sp.out.val_bytes) == (1, 17 + 8 + 9 + 8 + 9)
    assert sp.n_order == 2
    assert [(o.off, o.width, o.desc) for o in sp.order[:2]] == \
        [(0, 4, 1), (4, 4, 0)]
    assert sp.n_funcs == 4
    got = [(f.func, f.width, f.nullable, f.frame, f.off, f.has_default,
            f.offset, f.dflt) for f in sp.funcs[:4]]
    assert got == [
        (abi.MZ_WF_ROW_NUMBER, 0, 0, 0, 0, 0, 0, 0),
        (abi.MZ_WF_LAG, 8, 1, 0, 8, 1, 2, -5),
        (abi.MZ_WF_DENSE_RANK, 0, 0, 0, 0, 0, 0, 0),
        (abi.MZ_WF_LAST_VALUE, 4, 0, PART, 0, 0, 0, 0)]
    # a caller's out must be the derived one
    assert abi.window_spec(IN, ORDER, funcs,
                           out=abi.schema(1, 51)).out.val_bytes == 51


def test_builders():
    f = abi.wf_lead(4, 4)
    assert (f.func, f.off, f.width, f.offset, f.has_default, f.nullable) == \
        (abi.MZ_WF_LEAD, 4, 4, 1, 0, 0)
    f = abi.wf_lag(0, 8, 0, default=2**63 - 1)
    assert (f.offset, f.has_default, f.dflt) == (0, 1, 2**63 - 1)
    assert abi.wf_first_value(8, 8, nullable=1).nullable == 1
    assert abi.wf_last_value(8, 8).frame == abi.MZ_WF_FRAME_TO_CURRENT
    assert abi.wf_rank().func == abi.MZ_WF_RANK
    assert abi.wf_slot_bytes(abi.MZ_WF_RANK) == 8
    assert abi.wf_slot_bytes(abi.MZ_WF_FIRST_VALUE) == 9
    with pytest.raises(ValueError, match="u32"):
        abi.wf_lag(0, 8, -1)
    with pytest.raises(ValueError, match="i64"):
        abi.wf_lead(0, 8, 1, default=2**63)


def no_order_spec():
    sp = abi.window_spec(abi.schema(2, 0), [], [abi.wf_row_number()])
    assert (sp.out.key_words, sp.out.val_bytes, sp.n_order) == (2, 8, 0)


def bad_func(**kw):
    f = abi.wf_rank()
    for k, v in kw.items():
        setattr(f, k, v)
    return f


REFUSALS = {
    "varlen": (lambda: abi.window_spec(
        abi.schema(1, abi.MZ_GPU_VARLEN), [], [abi.wf_rank()]), "varlen"),
    "key_words": (lambda: abi.window_spec(
        abi.schema(3, 8), [], [abi.wf_rank()]), "key_words"),
    "no_funcs": (lambda: abi.window_spec(IN, ORDER, []), "n_funcs"),
    "five_funcs": (lambda: abi.window_spec(
        IN, ORDER, [abi.wf_rank()] * 5), "n_funcs"),
    "five_order": (lambda: abi.window_spec(
        IN, [(0, 4, False)] * 5, [abi.wf_rank()]), "n_order"),
    "order_width": (lambda: abi.window_spec(
        IN, [(0, 2, False)], [abi.wf_rank()]), "order column 0: width"),
    "order_past": (lambda: abi.window_spec(
        IN, [(0, 4, False), (10, 8, False)], [abi.wf_rank()]),
        "order column 1 reads past"),
    "datum_width": (lambda: abi.window_spec(
        IN, ORDER, [abi.wf_lag(0, 2)]), "func 0: datum width"),
    "datum_past": (lambda: abi.window_spec(
        IN, ORDER, [abi.wf_rank(), abi.wf_first_value(12, 8)]),
        "func 1 reads past"),
    # the datum fits, its null byte does not
    "null_byte_past": (lambda: abi.window_spec(
        abi.schema(1, 16), [], [abi.wf_lead(8, 8, nullable=1)]),
        "func 0 reads past"),
    "unknown_func": (lambda: abi.window_spec(
        IN, ORDER, [bad_func(func=7)]), "unknown func 7"),
    "unknown_frame": (lambda: abi.window_spec(
        IN, ORDER, [abi.wf_last_value(0, 4, frame=2)]), "unknown frame 2"),
    "frame_on_first_value": (lambda: abi.window_spec(
        IN, ORDER, [bad_func(func=abi.MZ_WF_FIRST_VALUE, width=4,
                             frame=PART)]), "LAST_VALUE only"),
    "frame_on_rank": (lambda: abi.window_spec(
        IN, ORDER, [bad_func(frame=PART)]), "LAST_VALUE only"),
    "out_too_wide": (lambda: abi.window_spec(
        abi.schema(1, 40), [], [abi.wf_lag(0, 8)] * 3), "more than 64"),
    "out_mismatch": (lambda: abi.window_spec(
        IN, ORDER, [abi.wf_rank()], out=abi.schema(1, 26)),
        "out schema must be 1 key words and 25 val bytes"),
    "out_key_mismatch": (lambda: abi.window_spec(
        IN, ORDER, [abi.wf_rank()], out=abi.schema(2, 25)),
        "out schema must be"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_create_time_refusals(name):
    fn, msg = REFUSALS[name]
    with pytest.raises(ValueError, match=msg):
        fn()


def test_legal_edges():
    no_order_spec()
    # exactly 64 out bytes; a nullable datum whose null byte is the last byte
    sp = abi.window_spec(abi.schema(1, 37), [(29, 8, True)],
                         [abi.wf_lag(28, 8, nullable=1)] * 3)
    assert sp.out.val_bytes == 64


def test_render_window_refuses_the_oracle():
    from pyoracle import OracleCtx
    sp = abi.window_spec(IN, ORDER, [abi.wf_rank()])
    with pytest.raises(NotImplementedError, match="window functions"):
        render.render_window(OracleCtx(), render.WindowPlan(sp))


def test_gpu_ctx_says_it_supports_window():
    from materialize_amd._ffi import GpuCtx
    assert GpuCtx.supports_window is True


LAYOUT_C = r"""
#include <stdio.h>
#include "mz_gpu.h"
int main(void) {
  printf("func %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
         sizeof(mz_gpu_window_func), offsetof(mz_gpu_window_func, func),
         offsetof(mz_gpu_window_func, width),
         offsetof(mz_gpu_window_func, nullable),
         offsetof(mz_gpu_window_func, frame),
         offsetof(mz_gpu_window_func, off),
         offsetof(mz_gpu_window_func, has_default),
         offsetof(mz_gpu_window_func, pad),
         offsetof(mz_gpu_window_func, offset),
         offsetof(mz_gpu_window_func, pad2),
         offsetof(mz_gpu_window_func, dflt));
  printf("spec %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mz_gpu_window_spec),
         offsetof(mz_gpu_window_spec, in),
         offsetof(mz_gpu_window_spec, n_order),
         offsetof(mz_gpu_window_spec, order),
         offsetof(mz_gpu_window_spec, n_funcs),
         offsetof(mz_gpu_window_spec, funcs),
         offsetof(mz_gpu_window_spec, out));
  printf("consts %d %d %d %d %d %d %d %d %d %d %d\n", MZ_GPU_MAX_WFUNCS,
         MZ_GPU_MAX_ORDER, MZ_WF_ROW_NUMBER, MZ_WF_RANK, MZ_WF_DENSE_RANK,
         MZ_WF_LAG, MZ_WF_LEAD, MZ_WF_FIRST_VALUE, MZ_WF_LAST_VALUE,
         MZ_WF_FRAME_TO_CURRENT, MZ_WF_FRAME_PARTITION);
  return 0;
}
"""


def test_ctypes_mirrors_match_the_header(tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True,
                           text=True).stdout.split("\n")
    func = [int(x) for x in lines[0].split()[1:]]
    spec = [int(x) for x in lines[1].split()[1:]]
    consts = [int(x) for x in lines[2].split()[1:]]
    F, S = abi.WindowFunc, abi.WindowSpec
    assert func == [abi.C.sizeof(F), F.func.offset, F.width.offset,
                    F.nullable.offset, F.frame.offset, F.off.offset,
                    F.has_default.offset, F.pad.offset, F.offset.offset,
                    F.pad2.offset, F.dflt.offset]
    assert func[0] == 24
    assert spec == [abi.C.sizeof(S), S.in_.offset, S.n_order.offset,
                    S.order.offset, S.n_funcs.offset, S.funcs.offset,
                    S.out.offset]
    assert consts == [abi.MZ_GPU_MAX_WFUNCS, abi.MZ_GPU_MAX_ORDER,
                      abi.MZ_WF_ROW_NUMBER, abi.MZ_WF_RANK,
                      abi.MZ_WF_DENSE_RANK, abi.MZ_WF_LAG, abi.MZ_WF_LEAD,
                      abi.MZ_WF_FIRST_VALUE, abi.MZ_WF_LAST_VALUE,
                      abi.MZ_WF_FRAME_TO_CURRENT, abi.MZ_WF_FRAME_PARTITION]
