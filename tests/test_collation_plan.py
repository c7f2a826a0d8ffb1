"""Collated reduce, CPU side: plan dispatch, spec layout, the Python-side
validation of the operator's restrictions, and the ctypes mirror of
mz_gpu_collation_spec against the C header."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from materialize_amd import _abi as abi
from materialize_amd import render

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def agg(func, off=0, width=8, nullable=0, is_float=0):
    return abi.Aggregate(func=func, off=off, width=width, is_float=is_float,
                         nullable=nullable)


COUNT = agg(abi.MZ_AGG_COUNT)
SUM_A = agg(abi.MZ_AGG_SUM_I64, 0)
MIN_B = agg(abi.AGG_MIN_I64, 8)
MAX_C = agg(abi.AGG_MAX_I64, 16, 4)


def test_function_ids_follow_sum_f64():
    assert abi.AGG_MIN_I64 == abi.MZ_AGG_SUM_F64 + 1
    assert abi.AGG_MAX_I64 == abi.MZ_AGG_SUM_F64 + 2


def test_plan_reduce_dispatch():
    sch = abi.schema(1, 24)
    p = render.plan_reduce([COUNT, SUM_A], sch)
    assert isinstance(p, render.ReducePlan)
    assert isinstance(p.spec, abi.ReduceSpec)
    p = render.plan_reduce([COUNT, SUM_A, MIN_B, MAX_C], sch)
    assert isinstance(p, render.CollationPlan)
    assert isinstance(p.spec, abi.CollationSpec)
    # a lone hierarchical aggregate is still a collation
    p = render.plan_reduce([MAX_C], sch, buckets=(16, 1))
    assert isinstance(p, render.CollationPlan)
    assert list(p.spec.buckets[:p.spec.n_levels]) == [16, 1]


def test_render_reduce_dispatch():
    class FakeCtx:
        def reduce_create(self, spec):
            return ("red", spec)

        def collation_create(self, spec):
            return ("col", spec)

    sch = abi.schema(1, 24)
    op = render.render_reduce(FakeCtx(), render.plan_reduce([COUNT], sch))
    assert isinstance(op, render.ReduceOp) and op.op[0] == "red"
    op = render.render_reduce(FakeCtx(),
                              render.plan_reduce([COUNT, MIN_B], sch))
    assert isinstance(op, render.CollationOp) and op.op[0] == "col"


def test_spec_layout():
    sp = abi.collation_spec([MIN_B, COUNT, MAX_C, SUM_A], abi.schema(2, 24))
    assert sp.n_aggs == 4
    assert [sp.aggs[i].func for i in range(4)] == [
        abi.AGG_MIN_I64, abi.MZ_AGG_COUNT, abi.AGG_MAX_I64,
        abi.MZ_AGG_SUM_I64]
    assert (sp.in_.key_words, sp.in_.val_bytes) == (2, 24)
    assert (sp.out.key_words, sp.out.val_bytes) == (2, 24 * 4)
    assert sp.n_levels == 3
    assert list(sp.buckets[:3]) == [256, 16, 1]
    # part 0 = the accumulable aggregates in their relative order, then one
    # part per MIN/MAX in spec order
    assert abi.collation_parts(sp) == [[1, 3], [0], [2]]
    sp = abi.collation_spec([MIN_B, MAX_C], abi.schema(1, 24), buckets=[1])
    assert abi.collation_parts(sp) == [[0], [1]]  # no part 0
    assert sp.out.val_bytes == 48


@pytest.mark.parametrize("aggs,sch,kw,match", [
    ([], abi.schema(1, 24), {}, "n_aggs"),
    ([COUNT] * 5, abi.schema(1, 24), {}, "n_aggs"),
    ([COUNT, MIN_B], abi.schema(1, abi.MZ_GPU_VARLEN), {}, "varlen"),
    ([COUNT, MIN_B], abi.schema(3, 24), {}, "key_words"),
    ([agg(abi.AGG_MIN_I64, 20, 8)], abi.schema(1, 24), {}, "reads past"),
    ([agg(abi.AGG_MAX_I64, 24, 4)], abi.schema(1, 24), {}, "reads past"),
    ([agg(abi.MZ_AGG_SUM_I64, 16, 8, nullable=1), MIN_B],
     abi.schema(1, 24), {}, "reads past"),
    ([agg(abi.AGG_MIN_I64, 0, 2)], abi.schema(1, 24), {}, "width"),
    ([agg(abi.AGG_MIN_I64, 0, 8, nullable=1)], abi.schema(1, 24), {},
     "nullable"),
    ([agg(7)], abi.schema(1, 24), {}, "unknown func"),
    ([COUNT, MIN_B], abi.schema(1, 24), {"buckets": ()}, "levels"),
    ([COUNT, MIN_B], abi.schema(1, 24), {"buckets": (64, 32, 16, 4, 1)},
     "levels"),
    ([COUNT, MIN_B], abi.schema(1, 24), {"buckets": (16, 4)}, "end with 1"),
    ([COUNT, MIN_B], abi.schema(1, 24), {"buckets": (0, 1)}, "positive"),
])
def test_validation_errors(aggs, sch, kw, match):
    with pytest.raises(ValueError, match=match):
        abi.collation_spec(aggs, sch, **kw)
    if any(abi.is_hierarchical(a) for a in aggs):
        with pytest.raises(ValueError, match=match):
            render.plan_reduce(aggs, sch, **kw)


def test_count_star_reads_nothing():
    # COUNT(*) carries no datum: it is valid over a val it could not index
    sp = abi.collation_spec([COUNT, agg(abi.AGG_MIN_I64, 0, 4)],
                            abi.schema(1, 4))
    assert sp.out.val_bytes == 48


def test_ctypes_struct_matches_header(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to read sizeof(mz_gpu_collation_spec)"
    src = tmp_path / "sz.cpp"
    src.write_text(
        '#include "mz_gpu.h"\n'
        '#include <cstdio>\n'
        '#include <cstddef>\n'
        'int main() { printf("%zu %zu %zu %zu\\n", '
        'sizeof(mz_gpu_collation_spec), offsetof(mz_gpu_collation_spec, in), '
        'offsetof(mz_gpu_collation_spec, n_levels), '
        'offsetof(mz_gpu_collation_spec, buckets)); }\n')
    exe = tmp_path / "sz"
    subprocess.run([cxx, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout.split()
    size, off_in, off_levels, off_buckets = map(int, out)
    assert C.sizeof(abi.CollationSpec) == size
    assert abi.CollationSpec.in_.offset == off_in
    assert abi.CollationSpec.n_levels.offset == off_levels
    assert abi.CollationSpec.buckets.offset == off_buckets
