"""Full-scan peek, CPU side: the render layer refuses contexts without the
scan peek, PeekPlan rejects closures a scan cannot evaluate before any
device call, and the opt-in Q3 output index is off by default."""
import pytest

from materialize_amd import _abi as abi
from materialize_amd import render
from materialize_amd.workloads import Q3Dataflow
from pyoracle import OracleCtx

KEY, VS, VL, CP = (abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_STREAM,
                   abi.MZ_SRC_VAL_LOOKUP, abi.MZ_SRC_COMPUTE)
SCH = abi.schema(1, 16)


def mfp(filters=(), key_fields=None, val_fields=None, out=None):
    return abi.closure(
        list(filters),
        [abi.field(KEY, 0, 8)] if key_fields is None else key_fields,
        [abi.field(VL, 0, 16)] if val_fields is None else val_fields,
        out or abi.schema(1, 16))


def test_gpu_ctx_declares_scan_peek():
    from materialize_amd._ffi import GpuCtx
    assert GpuCtx.supports_scan_peek is True  # class attribute, no device
    assert callable(GpuCtx.peek_scan) and callable(GpuCtx.peek_scan_dev)


def test_render_peek_refuses_context_without_scan_peek():
    o = OracleCtx()
    arr = o.arr_create(SCH)
    with pytest.raises(NotImplementedError, match="scan peek"):
        render.render_peek(o, arr, render.PeekPlan(SCH))


def test_valid_plans_construct():
    render.PeekPlan(SCH)
    render.PeekPlan(SCH, mfp(), allow_negative=True)
    # filter on a val field, projection, a computed i64 output field
    render.PeekPlan(SCH, mfp(
        [abi.filt(VL, 8, 8, abi.MZ_CMP_GT, 3)],
        val_fields=[abi.field(VL, 0, 8),
                    abi.field(CP, abi.MZ_COMPUTE_MUL_I64, 8, arg0=0, arg1=8,
                              arg0_src=VL, arg1_src=VL)]))
    render.PeekPlan(SCH, mfp(val_fields=[abi.field(VL, 8, 8)],
                             out=abi.schema(1, 8)))


@pytest.mark.parametrize("bad", [
    mfp([abi.filt(VS, 0, 8, abi.MZ_CMP_EQ, 0)]),
    mfp([abi.filt(CP, abi.MZ_COMPUTE_CMP_FIELDS, 8, abi.MZ_CMP_LT, 0,
                  arg0=0, arg1=8, arg0_src=VL, arg1_src=VS)]),
    mfp(key_fields=[abi.field(VS, 0, 8)]),
    mfp(val_fields=[abi.field(VS, 0, 16)]),
    mfp(val_fields=[abi.field(VL, 0, 8),
                    abi.field(CP, abi.MZ_COMPUTE_DIV_I64, 8, arg0=0, arg1=8,
                              arg0_src=VS, arg1_src=VL)]),
], ids=["filter", "filter-operand", "key-field", "val-field",
        "compute-operand"])
def test_plan_rejects_val_stream(bad):
    with pytest.raises(ValueError, match="MZ_SRC_VAL_STREAM"):
        render.PeekPlan(SCH, bad)


@pytest.mark.parametrize("bad", [
    mfp(val_fields=[abi.field(VL, 0, 8)]),                  # 8 != 16
    mfp(out=abi.schema(2, 16)),                             # key 8 != 16
    mfp(val_fields=[abi.field(VL, 0, 16),
                    abi.field(CP, abi.MZ_COMPUTE_MUL_I64, 8, arg0=0, arg1=8,
                              arg0_src=VL, arg1_src=VL)]),  # 24 != 16
], ids=["val-short", "key-short", "val-long"])
def test_plan_rejects_width_mismatch(bad):
    with pytest.raises(ValueError, match="out schema"):
        render.PeekPlan(SCH, bad)


def test_plan_rejects_varlen():
    with pytest.raises(ValueError, match="varlen"):
        render.PeekPlan(abi.schema(1, abi.MZ_GPU_VARLEN))


def test_q3_output_index_is_opt_in():
    df = Q3Dataflow(OracleCtx())  # default construction unchanged
    assert df.arr_out is None
    with pytest.raises(ValueError, match="index_output"):
        df.peek_result(0)
    with pytest.raises(NotImplementedError, match="scan peek"):
        Q3Dataflow(OracleCtx(), index_output=True)
