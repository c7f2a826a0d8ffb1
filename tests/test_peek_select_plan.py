"""Peek select, CPU side: the ctypes mirrors and builders of the key range
and the finishing, every refusal of include/mz_gpu.h by message (the rules
csrc/peek_select_spec.h states for the C layer), PeekPlan with and without
the new fields, and the render layer refusing contexts without the entry
point."""
import os
import shutil
import subprocess

import pytest

from materialize_amd import _abi as abi
from materialize_amd import render
from materialize_amd.workloads import Q3Dataflow, q3_top10
from pyoracle import OracleCtx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, VS, VL, CP = (abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_STREAM,
                   abi.MZ_SRC_VAL_LOOKUP, abi.MZ_SRC_COMPUTE)
NO_NULL = abi.MZ_GPU_NO_NULL
SCH = abi.schema(1, 16)


# ----------------------------------------------------- structs and builders

def test_struct_sizes():
    assert abi.C.sizeof(abi.KeyRange) == 40
    assert abi.C.sizeof(abi.PeekOrder) == 8
    assert abi.C.sizeof(abi.Finishing) == 56
    assert abi.C.sizeof(abi.PeekStats) == 16
    assert (abi.MZ_KB_UNBOUNDED, abi.MZ_KB_INCLUSIVE,
            abi.MZ_KB_EXCLUSIVE) == (0, 1, 2)
    assert NO_NULL == 0xFFFF


LAYOUT_C = r"""
#include <stdio.h>
#include "mz_gpu.h"
int main(void) {
  printf("range %zu %zu %zu %zu %zu\n", sizeof(mz_gpu_key_range),
         offsetof(mz_gpu_key_range, lo_kind),
         offsetof(mz_gpu_key_range, hi_kind), offsetof(mz_gpu_key_range, lo),
         offsetof(mz_gpu_key_range, hi));
  printf("order %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mz_gpu_peek_order),
         offsetof(mz_gpu_peek_order, src), offsetof(mz_gpu_peek_order, width),
         offsetof(mz_gpu_peek_order, desc),
         offsetof(mz_gpu_peek_order, nulls_last),
         offsetof(mz_gpu_peek_order, off),
         offsetof(mz_gpu_peek_order, null_off));
  printf("fin %zu %zu %zu %zu %zu\n", sizeof(mz_gpu_finishing),
         offsetof(mz_gpu_finishing, n_order),
         offsetof(mz_gpu_finishing, order),
         offsetof(mz_gpu_finishing, offset),
         offsetof(mz_gpu_finishing, limit));
  printf("stats %zu %zu %zu\n", sizeof(mz_gpu_peek_stats),
         offsetof(mz_gpu_peek_stats, scanned_vals),
         offsetof(mz_gpu_peek_stats, rows_matched));
  printf("consts %d %d %d %d %d\n", MZ_KB_UNBOUNDED, MZ_KB_INCLUSIVE,
         MZ_KB_EXCLUSIVE, (int)MZ_GPU_NO_NULL, MZ_GPU_MAX_ORDER);
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
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]]
           for ln in lines if ln}
    R, O, F, S = abi.KeyRange, abi.PeekOrder, abi.Finishing, abi.PeekStats
    sz = abi.C.sizeof
    assert got["range"] == [sz(R), R.lo_kind.offset, R.hi_kind.offset,
                            R.lo.offset, R.hi.offset]
    assert got["order"] == [sz(O), O.src.offset, O.width.offset,
                            O.desc.offset, O.nulls_last.offset, O.off.offset,
                            O.null_off.offset]
    assert got["fin"] == [sz(F), F.n_order.offset, F.order.offset,
                          F.offset.offset, F.limit.offset]
    assert got["stats"] == [sz(S), S.scanned_vals.offset,
                            S.rows_matched.offset]
    assert got["consts"] == [abi.MZ_KB_UNBOUNDED, abi.MZ_KB_INCLUSIVE,
                             abi.MZ_KB_EXCLUSIVE, NO_NULL,
                             abi.MZ_GPU_MAX_ORDER]


def test_key_range_builder():
    r = abi.key_range()
    assert (r.lo_kind, r.hi_kind) == (abi.MZ_KB_UNBOUNDED,) * 2
    assert list(r.lo) == list(r.hi) == [0, 0]
    r = abi.key_range(lo=-5, hi=9)
    assert (r.lo_kind, r.hi_kind) == (abi.MZ_KB_INCLUSIVE,) * 2
    assert (list(r.lo), list(r.hi)) == ([-5, 0], [9, 0])
    r = abi.key_range(lo=3, lo_inclusive=False)
    assert (r.lo_kind, r.hi_kind) == (abi.MZ_KB_EXCLUSIVE,
                                      abi.MZ_KB_UNBOUNDED)
    r = abi.key_range(hi=(1, -2**63), hi_inclusive=False, kw=2)
    assert (r.lo_kind, r.hi_kind) == (abi.MZ_KB_UNBOUNDED,
                                      abi.MZ_KB_EXCLUSIVE)
    assert list(r.hi) == [1, -2**63]
    r = abi.key_range(lo=-2**63, hi=2**63 - 1)
    assert (r.lo[0], r.hi[0]) == (-2**63, 2**63 - 1)
    abi.key_range(lo=9, hi=-9)  # lo > hi is the empty answer, not an error
    with pytest.raises(ValueError, match="takes 1 key words, not 2"):
        abi.key_range(lo=(1, 2))
    with pytest.raises(ValueError, match="takes 2 key words, not 1"):
        abi.key_range(hi=4, kw=2)
    with pytest.raises(ValueError, match="key_words must be 1 or 2"):
        abi.key_range(kw=3)


def test_order_by_builder_defaults():
    o = abi.order_by(VL, 4)
    assert (o.src, o.off, o.width, o.desc, o.nulls_last, o.null_off) == \
        (VL, 4, 8, 0, 1, NO_NULL)
    # the SQL default: NULLS LAST for ASC, NULLS FIRST for DESC
    assert abi.order_by(VL, 4, desc=True).nulls_last == 0
    assert abi.order_by(VL, 4, desc=True, nulls_last=True).nulls_last == 1
    assert abi.order_by(VL, 4, nulls_last=False).nulls_last == 0
    o = abi.order_by(VL, 8, width=16, desc=True, null_off=0)
    assert (o.width, o.desc, o.nulls_last, o.null_off) == (16, 1, 0, 0)
    o = abi.order_by(KEY, 8)
    assert (o.src, o.off, o.width, o.null_off) == (KEY, 8, 8, NO_NULL)


def test_finishing_builder_defaults():
    f = abi.finishing()
    assert (f.n_order, f.offset, f.limit) == (0, 0, -1)
    f = abi.finishing([abi.order_by(KEY, 0), abi.order_by(VL, 0, 4)],
                      limit=10, offset=3)
    assert (f.n_order, f.offset, f.limit) == (2, 3, 10)
    assert (f.order[1].src, f.order[1].width) == (VL, 4)
    assert abi.finishing(limit=0).limit == 0
    with pytest.raises(ValueError, match="n_order must be at most 4"):
        abi.finishing([abi.order_by(KEY, 0)] * 5)


# ------------------------------------------------- every refusal, by message

def raw_range(lk, lo, hk, hi):
    r = abi.KeyRange(lo_kind=lk, hi_kind=hk)
    r.lo[0], r.lo[1] = lo
    r.hi[0], r.hi[1] = hi
    return r


@pytest.mark.parametrize("r,kw,msg", [
    (raw_range(3, (0, 0), 1, (5, 0)), 1,
     "peek_select: range: unknown bound kind 3"),
    (raw_range(1, (0, 0), 255, (5, 0)), 1, "unknown bound kind 255"),
    (raw_range(1, (1, 7), 1, (5, 0)), 1,
     "nonzero bound word beyond key_words"),
    (raw_range(1, (1, 0), 2, (5, -1)), 1,
     "nonzero bound word beyond key_words"),
    (raw_range(0, (1, 0), 1, (5, 0)), 1,
     "nonzero bound word on an unbounded side"),
    (raw_range(1, (1, 0), 0, (0, 2)), 2,
     "nonzero bound word on an unbounded side"),
])
def test_range_refusals(r, kw, msg):
    assert msg in abi.peek_range_error(r, kw)
    with pytest.raises(ValueError, match=msg):
        render.PeekPlan(abi.schema(kw, 16), key_range=r)


def raw_order(src, off, width=8, null_off=NO_NULL, desc=0, nulls_last=0):
    return abi.PeekOrder(src=src, off=off, width=width, null_off=null_off,
                         desc=desc, nulls_last=nulls_last)


def raw_fin(cols):
    f = abi.Finishing(n_order=len(cols), limit=-1)
    for j, c in enumerate(cols[:abi.MZ_GPU_MAX_ORDER]):
        f.order[j] = c
    return f


# against an out row of 2 key words and 25 val bytes
ORDER_REFUSALS = [
    ([raw_order(KEY, 0)] * 5, "peek_select: n_order must be at most 4"),
    ([raw_order(VS, 0)],
     "order column 0: src must be MZ_SRC_KEY or MZ_SRC_VAL_LOOKUP"),
    ([raw_order(KEY, 0), raw_order(CP, 0)], "order column 1: src must be"),
    ([raw_order(KEY, 0, 4)], "order column 0: a key column must be width 8"),
    ([raw_order(KEY, 0, 16)], "a key column must be width 8"),
    ([raw_order(KEY, 4)],
     "a key column must sit at a word boundary inside the out key"),
    ([raw_order(KEY, 16)],
     "a key column must sit at a word boundary inside the out key"),
    ([raw_order(KEY, 0, 8, 0)], "a key column takes no null_off"),
    ([raw_order(VL, 0, 2)], "order column 0: width must be 4, 8 or 16"),
    ([raw_order(VL, 0, 0)], "width must be 4, 8 or 16"),
    ([raw_order(VL, 18)], "order column 0 reads past the out val"),
    ([raw_order(VL, 10, 16)], "reads past the out val"),
    ([raw_order(VL, 4, 8, 25)], "null_off is past the out val"),
    ([raw_order(VL, 4, 8, 4)], "null_off is inside its own datum"),
    ([raw_order(VL, 8, 16, 23)], "null_off is inside its own datum"),
    ([raw_order(VL, 4, 8, 12, desc=2)],
     "desc and nulls_last must be 0 or 1"),
    ([raw_order(KEY, 8, nulls_last=2)],
     "desc and nulls_last must be 0 or 1"),
]


@pytest.mark.parametrize("cols,msg", ORDER_REFUSALS,
                         ids=[m[-28:] + str(i)
                              for i, (_, m) in enumerate(ORDER_REFUSALS)])
def test_order_refusals(cols, msg):
    assert msg in abi.peek_finishing_error(raw_fin(cols), 2, 25)
    with pytest.raises(ValueError, match=msg):
        render.PeekPlan(abi.schema(2, 25), finishing=raw_fin(cols))


def test_builders_refuse_what_needs_no_schema():
    for kwargs, msg in (
            (dict(src=VS, off=0), "src must be"),
            (dict(src=KEY, off=0, width=4), "a key column must be width 8"),
            (dict(src=KEY, off=4), "word boundary"),
            (dict(src=KEY, off=0, null_off=3), "takes no null_off"),
            (dict(src=VL, off=0, width=2), "width must be 4, 8 or 16"),
            (dict(src=VL, off=4, null_off=11), "inside its own datum"),
            (dict(src=VL, off=4, desc=2), "desc and nulls_last")):
        with pytest.raises(ValueError, match=msg):
            abi.order_by(**kwargs)
    # the schema-dependent rules are the plan's
    far = abi.finishing([abi.order_by(VL, 100, null_off=99)])
    with pytest.raises(ValueError, match="order column 0 reads past"):
        render.PeekPlan(SCH, finishing=far)


def test_finishing_with_allow_negative_refused():
    msg = "a finishing cannot be combined with allow_negative"
    assert msg in abi.peek_finishing_error(abi.finishing(), 1, 16, True)
    with pytest.raises(ValueError, match=msg):
        render.PeekPlan(SCH, allow_negative=True, finishing=abi.finishing())
    # a range alone may see negative counts
    render.PeekPlan(SCH, allow_negative=True, key_range=abi.key_range(lo=1))


def test_legal_edges():
    ok = abi.peek_finishing_error
    assert ok(raw_fin([]), 1, 0) == ""
    assert ok(raw_fin([raw_order(KEY, 8, desc=1, nulls_last=1)]), 2, 0) == ""
    assert ok(raw_fin([raw_order(VL, 4, 8, 12)]), 1, 25) == ""
    assert ok(raw_fin([raw_order(VL, 8, 16, 0, desc=1)]), 2, 24) == ""
    assert ok(raw_fin([raw_order(VL, 21, 4), raw_order(VL, 9, 16, 8)]),
              1, 25) == ""
    assert ok(raw_fin([raw_order(VL, 0, 4, 24)]), 1, 25) == ""
    assert abi.peek_range_error(raw_range(2, (9, 0), 1, (-9, 0)), 1) == ""
    assert abi.peek_range_error(
        raw_range(1, (1, -2**63), 1, (1, 2**63 - 1)), 2) == ""


# ------------------------------------------------------------------ the plan

def test_plan_without_the_new_fields_is_the_scan_peek():
    p = render.PeekPlan(SCH)
    assert p.key_range is None and p.finishing is None and not p.selects
    p = render.PeekPlan(SCH, None, True)  # positional construction unchanged
    assert p.allow_negative and not p.selects


def test_plan_with_the_new_fields():
    fin = abi.finishing([abi.order_by(VL, 8, desc=True)], limit=10)
    assert render.PeekPlan(SCH, finishing=fin).selects
    assert render.PeekPlan(SCH, key_range=abi.key_range(lo=0)).selects
    # order columns address the mfp's OUT row: 8 val bytes here
    proj = abi.closure([], [abi.field(KEY, 0, 8)], [abi.field(VL, 8, 8)],
                       abi.schema(1, 8))
    render.PeekPlan(SCH, proj,
                    finishing=abi.finishing([abi.order_by(VL, 0)]))
    with pytest.raises(ValueError, match="reads past the out val"):
        render.PeekPlan(SCH, proj, finishing=fin)
    # ... and the range the STORED key: one word here, two out
    wide = abi.closure([], [abi.field(KEY, 0, 8), abi.field(VL, 0, 8)],
                       [abi.field(VL, 8, 8)], abi.schema(2, 8))
    render.PeekPlan(SCH, wide, key_range=abi.key_range(lo=1),
                    finishing=abi.finishing([abi.order_by(KEY, 8)]))
    with pytest.raises(ValueError, match="beyond key_words"):
        render.PeekPlan(SCH, wide, key_range=abi.key_range(lo=(1, 2), kw=2))


class ScanOnlyCtx:
    """A context with the full-scan peek alone."""
    supports_scan_peek = True


def test_render_peek_refuses_contexts_without_peek_select():
    fin = abi.finishing(limit=1)
    o = OracleCtx()
    arr = o.arr_create(SCH)
    with pytest.raises(NotImplementedError, match="peek select"):
        render.render_peek(o, arr, render.PeekPlan(SCH, finishing=fin))
    for plan in (render.PeekPlan(SCH, finishing=fin),
                 render.PeekPlan(SCH, key_range=abi.key_range(hi=3))):
        with pytest.raises(NotImplementedError, match=r"\(peek select\)"):
            render.render_peek(ScanOnlyCtx(), None, plan)
    render.render_peek(ScanOnlyCtx(), None, render.PeekPlan(SCH))


def test_gpu_ctx_declares_peek_select():
    from materialize_amd._ffi import GpuCtx
    assert GpuCtx.supports_peek_select is True  # class attribute, no device
    assert callable(GpuCtx.peek_select) and callable(GpuCtx.peek_select_dev)


def test_read_goes_through_peek_select_only_when_needed():
    calls = []

    class Ctx:
        supports_scan_peek = supports_peek_select = True

        def peek_scan_dev(self, *a):
            calls.append(("scan",) + a)

        def peek_select_dev(self, *a):
            calls.append(("select",) + a)

    fin, rng = abi.finishing(limit=2), abi.key_range(lo=1)
    render.render_peek(Ctx(), "arr", render.PeekPlan(SCH)).read(7)
    render.render_peek(Ctx(), "arr",
                       render.PeekPlan(SCH, key_range=rng,
                                       finishing=fin)).read(8)
    assert calls == [("scan", "arr", 7, None, False),
                     ("select", "arr", 8, rng, None, fin, False)]


def test_q3_top10_fits_the_output_index():
    fin = q3_top10()
    assert (fin.n_order, fin.limit, fin.offset) == (3, 10, 0)
    rev = fin.order[0]
    assert (rev.src, rev.off, rev.width, rev.desc, rev.null_off) == \
        (VL, 8, 16, 1, 0)
    render.PeekPlan(abi.schema(2, 24), finishing=fin)
    df = Q3Dataflow(OracleCtx())
    with pytest.raises(ValueError, match="index_output"):
        df.peek_result(0, finishing=fin)
