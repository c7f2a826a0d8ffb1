"""Temporal filter, CPU side: the binding surface exists, the render layer
refuses contexts without the operator, abi.time_bound lowers SQL comparators
the way MfpPlan::create_from does, abi.temporal_spec rejects the shapes the
operator refuses before any device call, and the ctypes structs lay out
exactly as include/mz_gpu.h does."""
import ctypes as C
import os
import subprocess

import pytest

from materialize_amd import _abi as abi
from materialize_amd import render
from pyoracle import OracleCtx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, VS, VL, CP = (abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_STREAM,
                   abi.MZ_SRC_VAL_LOOKUP, abi.MZ_SRC_COMPUTE)
LOWER, UPPER = abi.MZ_TB_LOWER, abi.MZ_TB_UPPER
SCH = abi.schema(1, 16)
WINDOW = (abi.time_bound(abi.MZ_CMP_GE, VS, 0)
          + abi.time_bound(abi.MZ_CMP_LT, VS, 0, add=30000))


def mfp(filters=(), key_fields=None, val_fields=None, out=None):
    return abi.closure(
        list(filters),
        [abi.field(KEY, 0, 8)] if key_fields is None else key_fields,
        [abi.field(VS, 0, 16)] if val_fields is None else val_fields,
        out or abi.schema(1, 16))


def test_gpu_ctx_declares_temporal_filter():
    from materialize_amd._ffi import GpuCtx
    assert GpuCtx.supports_temporal_filter is True  # class attr, no device
    for name in ("temporal_create", "temporal_push", "temporal_push_dev",
                 "temporal_stats", "temporal_drop"):
        assert callable(getattr(GpuCtx, name)), name
    assert abi.MZ_GPU_MAX_BOUNDS == 4
    assert abi.MZ_ERR_TIMESTAMP_OUT_OF_RANGE == 2
    assert (LOWER, UPPER) == (0, 1)


def test_render_refuses_context_without_temporal_filter():
    plan = render.TemporalFilterPlan(abi.temporal_spec(SCH, WINDOW))
    with pytest.raises(NotImplementedError, match="temporal filter"):
        render.render_temporal_filter(OracleCtx(), plan)


@pytest.mark.parametrize("cmp, want", [
    (abi.MZ_CMP_GE, [(LOWER, 7)]),
    (abi.MZ_CMP_GT, [(LOWER, 8)]),
    (abi.MZ_CMP_LT, [(UPPER, 7)]),
    (abi.MZ_CMP_LE, [(UPPER, 8)]),
    (abi.MZ_CMP_EQ, [(LOWER, 7), (UPPER, 8)]),
], ids=["ge", "gt", "lt", "le", "eq"])
def test_time_bound_lowering(cmp, want):
    got = abi.time_bound(cmp, VS, 4, width=4, add=7, nullable=1)
    assert [(b.kind, b.add) for b in got] == want
    for b in got:
        assert (b.src, b.off, b.width, b.nullable) == (VS, 4, 4, 1)
    # defaults: 8 bytes, add 0, not nullable
    d = abi.time_bound(cmp, KEY, 0)
    assert [(b.kind, b.add) for b in d] == [(k, a - 7) for k, a in want]
    assert all((b.src, b.width, b.nullable) == (KEY, 8, 0) for b in d)


def test_time_bound_rejects_ne():
    with pytest.raises(ValueError, match="not a temporal predicate"):
        abi.time_bound(abi.MZ_CMP_NE, VS, 0)


def test_valid_specs_construct():
    sp = abi.temporal_spec(SCH, WINDOW)
    assert (sp.has_mfp, sp.n_bounds, sp.until) == (0, 2, 2**64 - 1)
    assert [(b.kind, b.add) for b in sp.bounds[:2]] == [(LOWER, 0),
                                                        (UPPER, 30000)]
    # a list of lists, an mfp with a filter, a projection and a computed
    # field, until and a capacity hint
    sp = abi.temporal_spec(
        SCH, [abi.time_bound(abi.MZ_CMP_EQ, KEY, 0),
              abi.TimeBound(kind=UPPER, src=VS, off=8, width=4, add=-3)],
        mfp=mfp([abi.filt(VS, 8, 8, abi.MZ_CMP_GT, 3)],
                val_fields=[abi.field(CP, abi.MZ_COMPUTE_MUL_I64, 8, arg0=0,
                                      arg1=8, arg0_src=VS, arg1_src=VS)],
                out=abi.schema(1, 8)),
        until=100, initial_rows=8)
    assert (sp.has_mfp, sp.n_bounds, sp.until, sp.initial_rows) == \
        (1, 3, 100, 8)
    assert sp.mfp.out.val_bytes == 8
    render.TemporalFilterPlan(sp)


B = abi.TimeBound
BAD_SPECS = {
    "varlen": (abi.schema(1, abi.MZ_GPU_VARLEN), WINDOW, None, "varlen"),
    "no-bounds": (SCH, [], None, "n_bounds"),
    "five-bounds": (SCH, WINDOW + WINDOW + WINDOW[:1], None, "n_bounds"),
    "bound-past-val": (SCH, [B(kind=LOWER, src=VS, off=12, width=8)], None,
                       "out of range"),
    "bound-null-byte-past-val": (
        SCH, [B(kind=LOWER, src=VS, off=8, width=8, nullable=1)], None,
        "out of range"),
    "bound-past-key": (SCH, [B(kind=UPPER, src=KEY, off=8, width=4)], None,
                       "out of range"),
    "bound-from-lookup": (SCH, [B(kind=LOWER, src=VL, off=0, width=8)], None,
                          "MZ_SRC_KEY or MZ_SRC_VAL_STREAM"),
    "bound-width": (SCH, [B(kind=LOWER, src=VS, off=0, width=2)], None,
                    "width"),
    "bound-kind": (SCH, [B(kind=2, src=VS, off=0, width=8)], None, "kind"),
    "mfp-filter-lookup": (SCH, WINDOW,
                          mfp([abi.filt(VL, 0, 8, abi.MZ_CMP_EQ, 0)]),
                          "MZ_SRC_VAL_LOOKUP"),
    "mfp-field-lookup": (SCH, WINDOW,
                         mfp(val_fields=[abi.field(VL, 0, 16)]),
                         "MZ_SRC_VAL_LOOKUP"),
    "mfp-operand-lookup": (
        SCH, WINDOW,
        mfp(val_fields=[abi.field(VS, 0, 8),
                        abi.field(CP, abi.MZ_COMPUTE_MUL_I64, 8, arg0=0,
                                  arg1=8, arg0_src=VS, arg1_src=VL)]),
        "MZ_SRC_VAL_LOOKUP"),
    "mfp-div": (
        SCH, WINDOW,
        mfp(val_fields=[abi.field(VS, 0, 8),
                        abi.field(CP, abi.MZ_COMPUTE_DIV_I64, 8, arg0=0,
                                  arg1=8, arg0_src=VS, arg1_src=VS)]),
        "MZ_COMPUTE_DIV_I64"),
    "mfp-filter-past-val": (SCH, WINDOW,
                            mfp([abi.filt(VS, 12, 8, abi.MZ_CMP_EQ, 0)]),
                            "out of range"),
    "mfp-field-past-val": (SCH, WINDOW,
                           mfp(val_fields=[abi.field(VS, 8, 16)]),
                           "out of range"),
    "mfp-width-mismatch": (SCH, WINDOW,
                           mfp(val_fields=[abi.field(VS, 0, 8)]),
                           "out schema"),
    "mfp-out-too-wide": (
        abi.schema(1, 64), WINDOW,
        mfp(val_fields=[abi.field(VS, 0, 64), abi.field(VS, 0, 8)],
            out=abi.schema(1, 72)),
        "wider"),
    "mfp-out-three-key-words": (
        SCH, WINDOW,
        mfp(key_fields=[abi.field(KEY, 0, 8), abi.field(VS, 0, 16)],
            out=abi.schema(3, 16)),
        "wider"),
}


@pytest.mark.parametrize("name", sorted(BAD_SPECS))
def test_spec_rejects(name):
    sch, bounds, m, msg = BAD_SPECS[name]
    with pytest.raises(ValueError, match=msg):
        abi.temporal_spec(sch, bounds, mfp=m)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mz_gpu.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  S(mz_gpu_time_bound);
  O(mz_gpu_time_bound, kind); O(mz_gpu_time_bound, src);
  O(mz_gpu_time_bound, off); O(mz_gpu_time_bound, width);
  O(mz_gpu_time_bound, nullable); O(mz_gpu_time_bound, add);
  S(mz_gpu_temporal_spec);
  O(mz_gpu_temporal_spec, in); O(mz_gpu_temporal_spec, has_mfp);
  O(mz_gpu_temporal_spec, mfp); O(mz_gpu_temporal_spec, n_bounds);
  O(mz_gpu_temporal_spec, bounds); O(mz_gpu_temporal_spec, until);
  O(mz_gpu_temporal_spec, initial_rows);
  printf("MZ_GPU_MAX_BOUNDS %d\n", MZ_GPU_MAX_BOUNDS);
  printf("MZ_TB_LOWER %d\nMZ_TB_UPPER %d\n", MZ_TB_LOWER, MZ_TB_UPPER);
  printf("MZ_ERR_TIMESTAMP_OUT_OF_RANGE %d\n", MZ_ERR_TIMESTAMP_OUT_OF_RANGE);
  return 0;
}
"""


def test_struct_layout_matches_header(tmp_path):
    """A mismatch here corrupts every call silently: compile a host-only C
    program against the header and compare sizeof/offsetof with ctypes."""
    src = tmp_path / "layout.c"
    exe = tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99",
                    "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout
    c_side = dict(line.rsplit(" ", 1) for line in out.splitlines())
    c_side = {k: int(v) for k, v in c_side.items()}
    want = {"MZ_GPU_MAX_BOUNDS": abi.MZ_GPU_MAX_BOUNDS,
            "MZ_TB_LOWER": LOWER, "MZ_TB_UPPER": UPPER,
            "MZ_ERR_TIMESTAMP_OUT_OF_RANGE":
                abi.MZ_ERR_TIMESTAMP_OUT_OF_RANGE}
    for cname, ty in (("mz_gpu_time_bound", abi.TimeBound),
                      ("mz_gpu_temporal_spec", abi.TemporalSpec)):
        want[cname] = C.sizeof(ty)
        for fname, _ in ty._fields_:
            want[f"{cname}.{fname.rstrip('_')}"] = getattr(ty, fname).offset
    assert c_side == want
