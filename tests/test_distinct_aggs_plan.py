"""DISTINCT aggregates (COUNT/SUM DISTINCT), CPU side: the `distinct` byte of
mz_gpu_aggregate against the C header, plan dispatch, the Python-side
validation of the rejected shapes, and the render layer's refusal to run a
DISTINCT plan on a context that does not implement it."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def agg(func, off=0, width=8, nullable=0, is_float=0, distinct=0):
    return abi.Aggregate(func=func, off=off, width=width, is_float=is_float,
                         nullable=nullable, distinct=distinct)


COUNT = agg(abi.MZ_AGG_COUNT)
SUM_A = agg(abi.MZ_AGG_SUM_I64, 0)
COUNT_D_A = agg(abi.MZ_AGG_COUNT, 0, distinct=1)
SUM_D_C = agg(abi.MZ_AGG_SUM_I64, 16, 4, distinct=1)
MIN_B = agg(abi.AGG_MIN_I64, 8)


def test_ctypes_aggregate_matches_header(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to read sizeof(mz_gpu_aggregate)"
    src = tmp_path / "sz.cpp"
    src.write_text(
        '#include "mz_gpu.h"\n'
        '#include <cstdio>\n'
        '#include <cstddef>\n'
        'int main() { printf("%zu %zu %zu %zu\\n", '
        'sizeof(mz_gpu_aggregate), offsetof(mz_gpu_aggregate, distinct), '
        'sizeof(mz_gpu_reduce_spec), sizeof(mz_gpu_collation_spec)); }\n')
    exe = tmp_path / "sz"
    subprocess.run([cxx, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout.split()
    size, off_distinct, size_red, size_col = map(int, out)
    assert size == 8 and off_distinct == 7  # the former padding byte
    assert C.sizeof(abi.Aggregate) == size
    assert abi.Aggregate.distinct.offset == off_distinct
    # the specs that embed the aggregate keep their layout
    assert C.sizeof(abi.ReduceSpec) == size_red == 52
    assert C.sizeof(abi.CollationSpec) == size_col == 72


def test_distinct_defaults_to_plain():
    a = abi.Aggregate(func=abi.MZ_AGG_SUM_I64, off=0, width=8, is_float=0,
                      nullable=0)
    assert a.distinct == 0 and not abi.is_distinct(a)
    assert abi.is_distinct(COUNT_D_A)
    # MIN/MAX carry the flag without effect
    assert not abi.is_distinct(agg(abi.AGG_MIN_I64, 8, distinct=1))


def test_plan_reduce_keeps_flag():
    sch = abi.schema(1, 24)
    p = render.plan_reduce([COUNT_D_A, SUM_D_C, COUNT, SUM_A], sch)
    assert isinstance(p, render.ReducePlan)
    assert [p.spec.aggs[i].distinct for i in range(4)] == [1, 1, 0, 0]
    assert (p.spec.aggs[1].off, p.spec.aggs[1].width) == (16, 4)
    p = render.plan_reduce([COUNT_D_A, MIN_B, SUM_A], sch, buckets=(16, 1))
    assert isinstance(p, render.CollationPlan)
    assert [p.spec.aggs[i].distinct for i in range(3)] == [1, 0, 0]
    # MIN/MAX accept the flag
    p = render.plan_reduce([agg(abi.AGG_MAX_I64, 8, distinct=1), COUNT], sch)
    assert isinstance(p, render.CollationPlan)
    assert p.spec.aggs[0].distinct == 1


REJECTED = [
    (agg(abi.MZ_AGG_SUM_F64, 0, 8, is_float=1, distinct=1), 24, "float"),
    (agg(abi.MZ_AGG_SUM_I64, 0, 8, is_float=1, distinct=1), 24, "float"),
    (agg(abi.MZ_AGG_COUNT, 0, 8, is_float=1, distinct=1), 24, "float"),
    (agg(abi.MZ_AGG_COUNT, 0, 2, distinct=1), 24, "width"),
    (agg(abi.MZ_AGG_COUNT, 0, 0, distinct=1), 24, "width"),
    (agg(abi.MZ_AGG_COUNT, 20, 8, distinct=1), 24, "reads past"),
    (agg(abi.MZ_AGG_COUNT, 16, 8, nullable=1, distinct=1), 24, "reads past"),
    (agg(abi.MZ_AGG_SUM_I64, 24, 4, distinct=1), 24, "reads past"),
]


@pytest.mark.parametrize("a,vb,match", REJECTED)
def test_rejected_shapes(a, vb, match):
    sch = abi.schema(1, vb)
    with pytest.raises(ValueError, match=match):
        abi.reduce_spec([a], sch)
    with pytest.raises(ValueError, match=match):
        abi.collation_spec([a, MIN_B], sch)
    with pytest.raises(ValueError, match=match):
        render.plan_reduce([COUNT, a], sch)
    with pytest.raises(ValueError, match=match):
        render.plan_reduce([a, MIN_B], sch)


def test_same_shapes_pass_without_the_flag():
    # the checks belong to DISTINCT: a plain COUNT(*) reads nothing
    sch = abi.schema(1, 4)
    abi.reduce_spec([agg(abi.MZ_AGG_COUNT, 20, 8)], sch)
    abi.reduce_spec([agg(abi.MZ_AGG_SUM_F64, 0, 8, is_float=1)],
                    abi.schema(1, 8))


def updates(keys, a, diffs, t):
    vals = np.zeros((len(keys), 3), np.int64)
    vals[:, 0] = a
    return abi.make_updates(np.asarray(keys, np.int64),
                            vals.view(np.uint8).ravel(),
                            np.full(len(keys), t, np.uint64),
                            np.asarray(diffs, np.int64), t, t + 1)


def test_oracle_context_refuses_distinct():
    from pyoracle import OracleCtx
    ctx = OracleCtx()
    assert not getattr(ctx, "supports_distinct_aggs", False)
    sch = abi.schema(1, 24)
    with pytest.raises(NotImplementedError, match="DISTINCT"):
        render.render_reduce(ctx, render.plan_reduce([COUNT_D_A, SUM_A], sch))
    with pytest.raises(NotImplementedError, match="DISTINCT"):
        render.render_reduce(
            ctx, render.plan_reduce([COUNT_D_A, MIN_B], sch, buckets=(16, 1)))
    # the same plan without the flag still renders and runs
    op = render.render_reduce(
        ctx, render.plan_reduce([agg(abi.MZ_AGG_COUNT, 0), SUM_A], sch))
    out = op.push(updates([1, 1, 2], [5, 5, 7], [1, 1, 1], 0))
    keys, vals, _, diffs = out.to_host()
    assert list(keys) == [1, 2] and list(diffs) == [1, 1]
    counts = vals.reshape(2, 48)[:, 8:16].copy().view(np.int64).ravel()
    assert list(counts) == [2, 1]  # plain COUNT: the duplicate counts


def test_gpu_context_advertises_distinct():
    # the class attribute: no device is touched
    from materialize_amd._ffi import GpuCtx
    assert GpuCtx.supports_distinct_aggs is True
