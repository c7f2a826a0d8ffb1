"""Window aggregates (SUM / COUNT / MIN / MAX OVER), the parts that need no
GPU: the builders, slot sizes and derived out schemas for mixes of old and
new functions, every create-time refusal by message, the legal edges, the
expansion rule, the ctypes mirror against the C header (new constants and
the union field names included), and the C layer's own spec checker built
as a stand-alone host program."""
import os
import shutil
import subprocess

import pytest

from materialize_amd import _abi as abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN = abi.schema(1, 17)  # a i32 @0, b i32 @4, x i64 @8 with null byte @16
ORDER = [(0, 4, True), (4, 4, False)]
TO_CUR, PART, ROWS = (abi.MZ_WF_FRAME_TO_CURRENT, abi.MZ_WF_FRAME_PARTITION,
                      abi.MZ_WF_FRAME_ROWS)
UP, CUR, UF = abi.UNBOUNDED_PRECEDING, abi.CURRENT_ROW, abi.UNBOUNDED_FOLLOWING
P, F = abi.preceding, abi.following
X = dict(off=8, width=8, nullable=1)


def test_constants():
    assert (abi.MZ_WF_SUM, abi.MZ_WF_COUNT, abi.MZ_WF_MIN, abi.MZ_WF_MAX) == \
        (16, 17, 18, 19)
    assert ROWS == 2
    assert (abi.MZ_WB_UNBOUNDED_PRECEDING, abi.MZ_WB_PRECEDING,
            abi.MZ_WB_CURRENT_ROW, abi.MZ_WB_FOLLOWING,
            abi.MZ_WB_UNBOUNDED_FOLLOWING) == (0, 1, 2, 3, 4)


def test_builders():
    f = abi.wf_sum(8, 8)
    assert (f.func, f.off, f.width, f.nullable, f.frame, f.bounds, f.offset,
            f.end_offset, f.has_default, f.dflt) == \
        (abi.MZ_WF_SUM, 8, 8, 0, TO_CUR, 0, 0, 0, 0, 0)  # the SQL default
    f = abi.wf_count()
    assert (f.func, f.off, f.width, f.nullable, f.frame) == \
        (abi.MZ_WF_COUNT, 0, 0, 0, TO_CUR)
    f = abi.wf_min(frame=PART, **X)
    assert (f.func, f.frame, f.nullable, f.bounds) == \
        (abi.MZ_WF_MIN, PART, 1, 0)
    f = abi.wf_max(0, 4, start=P(2), end=UF)
    assert (f.func, f.frame, f.bounds, f.offset, f.end_offset) == \
        (abi.MZ_WF_MAX, ROWS,
         abi.MZ_WB_PRECEDING | abi.MZ_WB_UNBOUNDED_FOLLOWING << 4, 2, 0)
    # the reused bytes: second names of pad / pad2
    assert (f.pad, f.pad2) == (f.bounds, f.end_offset)
    f = abi.wf_sum(8, 8, start=P(3), end=F(7))
    assert (f.bounds, f.offset, f.end_offset, f.pad2) == (1 | 3 << 4, 3, 7, 7)
    # one bound given: the other is the SQL default for it
    f = abi.wf_count(start=CUR)
    assert (f.frame, f.bounds) == (ROWS, 2 | 2 << 4)
    f = abi.wf_count(end=UF)
    assert (f.frame, f.bounds) == (ROWS, 0 | 4 << 4)
    assert abi.wf_sum(8, 8, frame=ROWS, start=UP, end=UF).frame == ROWS
    with pytest.raises(ValueError, match="need MZ_WF_FRAME_ROWS"):
        abi.wf_sum(8, 8, frame=PART, start=CUR)
    with pytest.raises(ValueError, match="u32"):
        abi.wf_sum(8, 8, start=P(-1))
    with pytest.raises(ValueError, match="u32"):
        abi.wf_sum(8, 8, end=F(2**32))


def test_slot_sizes():
    assert abi.wf_slot_bytes(abi.MZ_WF_COUNT) == 8
    for func in (abi.MZ_WF_SUM, abi.MZ_WF_MIN, abi.MZ_WF_MAX):
        assert abi.wf_slot_bytes(func) == 9
        assert abi.wf_is_value(func) and abi.wf_is_agg(func)
    assert abi.wf_is_agg(abi.MZ_WF_COUNT)
    assert not abi.wf_is_value(abi.MZ_WF_COUNT)
    assert not abi.wf_is_agg(abi.MZ_WF_LAST_VALUE)
    # unchanged for the others
    assert [abi.wf_slot_bytes(f) for f in range(7)] == [8, 8, 8, 9, 9, 9, 9]


def test_out_schema_of_mixes():
    funcs = [abi.wf_row_number(), abi.wf_sum(**X),
             abi.wf_count(), abi.wf_lag(8, 8, 1, nullable=1)]
    sp = abi.window_spec(IN, ORDER, funcs)
    assert (sp.out.key_words, sp.out.val_bytes) == (1, 17 + 8 + 9 + 8 + 9)
    assert [f.func for f in sp.funcs[:4]] == \
        [abi.MZ_WF_ROW_NUMBER, abi.MZ_WF_SUM, abi.MZ_WF_COUNT, abi.MZ_WF_LAG]
    funcs = [abi.wf_min(0, 4, frame=PART), abi.wf_max(4, 4),
             abi.wf_count(**X), abi.wf_last_value(0, 4, frame=PART)]
    sp = abi.window_spec(IN, ORDER, funcs)
    assert sp.out.val_bytes == 17 + 9 + 9 + 8 + 9
    got = [(f.func, f.width, f.nullable, f.frame, f.off, f.bounds, f.offset,
            f.end_offset) for f in sp.funcs[:3]]
    assert got == [(abi.MZ_WF_MIN, 4, 0, PART, 0, 0, 0, 0),
                   (abi.MZ_WF_MAX, 4, 0, TO_CUR, 4, 0, 0, 0),
                   (abi.MZ_WF_COUNT, 8, 1, TO_CUR, 8, 0, 0, 0)]
    sp = abi.window_spec(abi.schema(2, 0), [], [abi.wf_count()])
    assert (sp.out.key_words, sp.out.val_bytes) == (2, 8)
    assert abi.window_spec(IN, ORDER, [abi.wf_sum(**X)],
                           out=abi.schema(1, 26)).out.val_bytes == 26


def edited(f, **kw):
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def spec1(f, in_schema=IN):
    return lambda: abi.window_spec(in_schema, ORDER, [f])


REFUSALS = {
    "agg_frame_3": (spec1(abi.wf_sum(frame=3, **X)),
                    "func 0: unknown frame 3"),
    # MZ_WF_FRAME_ROWS is the aggregates' alone
    "rows_on_last_value": (spec1(abi.wf_last_value(0, 4, frame=ROWS)),
                           "unknown frame 2"),
    "rows_on_first_value": (spec1(edited(abi.wf_first_value(0, 4),
                                         frame=ROWS)), "LAST_VALUE only"),
    "rows_on_rank": (spec1(edited(abi.wf_rank(), frame=ROWS)),
                     "LAST_VALUE only"),
    "rows_on_lag": (spec1(edited(abi.wf_lag(0, 4), frame=ROWS)),
                    "LAST_VALUE only"),
    "frame_3_on_rank": (spec1(edited(abi.wf_rank(), frame=3)),
                        "unknown frame 3"),
    "unknown_func_15": (spec1(edited(abi.wf_rank(), func=15)),
                        "unknown func 15"),
    "unknown_func_20": (spec1(edited(abi.wf_rank(), func=20)),
                        "unknown func 20"),
    "start_kind": (spec1(abi.wf_sum(start=(5, 0), end=CUR, **X)),
                   "unknown bound kind 5"),
    "end_kind": (spec1(abi.wf_sum(start=CUR, end=(15, 0), **X)),
                 "unknown bound kind 15"),
    "start_unbounded_following": (spec1(abi.wf_sum(start=UF, end=UF, **X)),
                                  "cannot start at UNBOUNDED FOLLOWING"),
    "end_unbounded_preceding": (spec1(abi.wf_sum(start=UP, end=UP, **X)),
                                "cannot end at UNBOUNDED PRECEDING"),
    "current_to_preceding": (spec1(abi.wf_count(start=CUR, end=P(1))),
                             "starting at CURRENT ROW cannot end PRECEDING"),
    "following_to_preceding": (
        spec1(abi.wf_sum(start=F(1), end=P(1), **X)),
        "starting FOLLOWING cannot end PRECEDING or at CURRENT ROW"),
    "following_to_current": (
        spec1(abi.wf_sum(start=F(1), end=CUR, **X)),
        "starting FOLLOWING cannot end PRECEDING or at CURRENT ROW"),
    "bounds_without_rows": (spec1(edited(abi.wf_sum(**X), bounds=2 | 4 << 4)),
                            "bounds and offsets need MZ_WF_FRAME_ROWS"),
    "offset_without_rows": (spec1(edited(abi.wf_sum(frame=PART, **X),
                                         offset=1)),
                            "bounds and offsets need MZ_WF_FRAME_ROWS"),
    "end_offset_without_rows": (spec1(edited(abi.wf_count(), end_offset=1)),
                                "bounds and offsets need MZ_WF_FRAME_ROWS"),
    "offset_on_current_row": (spec1(abi.wf_sum(start=(2, 3), end=UF, **X)),
                              "an offset on an UNBOUNDED or CURRENT ROW"),
    "sum_width_0": (spec1(abi.wf_sum(8, 0)), "datum width must be 4 or 8"),
    "min_width_2": (spec1(abi.wf_min(8, 2)), "datum width must be 4 or 8"),
    "count_width_2": (spec1(abi.wf_count(8, 2)),
                      r"datum width must be 4 or 8, or 0 for COUNT\(\*\)"),
    "count_star_with_offset": (spec1(abi.wf_count(8, 0)),
                               r"COUNT\(\*\) takes no datum"),
    "datum_past": (spec1(abi.wf_sum(12, 8)), "func 0 reads past"),
    # the datum fits, its null byte does not
    "null_byte_past": (spec1(abi.wf_max(8, 8, nullable=1),
                             abi.schema(1, 16)), "func 0 reads past"),
    "has_default": (spec1(edited(abi.wf_sum(**X), has_default=1)),
                    "an aggregate takes no default"),
    "dflt": (spec1(edited(abi.wf_min(**X), dflt=-1)),
             "an aggregate takes no default"),
    "min_two_sided": (spec1(abi.wf_min(start=P(1), end=F(1), **X)),
                      "MIN / MAX over a ROWS frame bounded on both sides is "
                      "not provided"),
    "max_current_row_only": (spec1(abi.wf_max(start=CUR, end=CUR, **X)),
                             "range-minimum structure"),
    "out_too_wide": (lambda: abi.window_spec(
        abi.schema(1, 40), [], [abi.wf_sum(0, 8)] * 3), "more than 64"),
    "out_mismatch": (lambda: abi.window_spec(
        IN, ORDER, [abi.wf_count()], out=abi.schema(1, 26)),
        "out schema must be 1 key words and 25 val bytes"),
    "five_funcs": (lambda: abi.window_spec(IN, ORDER, [abi.wf_count()] * 5),
                   "n_funcs"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_create_time_refusals(name):
    fn, msg = REFUSALS[name]
    with pytest.raises(ValueError, match=msg):
        fn()


def test_legal_edges():
    # COUNT(*) needs no val at all
    sp = abi.window_spec(abi.schema(1, 0), [], [abi.wf_count()])
    assert sp.out.val_bytes == 8 and sp.funcs[0].width == 0
    # exactly 64 out bytes; a nullable datum whose null byte is the last byte
    sp = abi.window_spec(abi.schema(1, 37), [(29, 8, True)],
                         [abi.wf_sum(28, 8, nullable=1),
                          abi.wf_min(28, 8, nullable=1),
                          abi.wf_max(28, 8, nullable=1)])
    assert sp.out.val_bytes == 64
    # k PRECEDING .. k' PRECEDING is legal for any k, k': this one is empty
    sp = abi.window_spec(IN, ORDER, [abi.wf_sum(start=P(3), end=P(5), **X)])
    assert (sp.funcs[0].offset, sp.funcs[0].end_offset) == (3, 5)
    abi.window_spec(IN, ORDER, [abi.wf_count(start=F(5), end=F(3))])
    # MIN / MAX with one unbounded end, on either side
    abi.window_spec(IN, ORDER, [abi.wf_min(start=UP, end=F(2), **X),
                                abi.wf_max(start=P(2), end=UF, **X),
                                abi.wf_min(start=UP, end=UF, **X),
                                abi.wf_max(start=UP, end=CUR, **X)])


def test_expansion_rule():
    assert abi.wf_expands(abi.wf_sum(start=P(1), end=F(1), **X))
    assert abi.wf_expands(abi.wf_count(start=UP, end=CUR))
    assert abi.wf_expands(abi.wf_max(start=CUR, end=UF, **X))
    # both ends unbounded is the whole partition
    assert not abi.wf_expands(abi.wf_sum(start=UP, end=UF, **X))
    assert not abi.wf_expands(abi.wf_sum(**X))
    assert not abi.wf_expands(abi.wf_min(frame=PART, **X))
    assert abi.wf_expands(abi.wf_row_number())
    assert abi.wf_expands(abi.wf_lead(0, 4))
    assert not abi.wf_expands(abi.wf_rank())
    assert not abi.wf_expands(abi.wf_last_value(0, 4))


def compiler(names):
    return next((c for c in names if shutil.which(c)), None)


LAYOUT_C = r"""
#include <stdio.h>
#include "mz_gpu.h"
int main(void) {
  mz_gpu_window_func f = {0};
  f.bounds = 0x42;
  f.end_offset = 7;
  printf("func %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n",
         sizeof(mz_gpu_window_func), offsetof(mz_gpu_window_func, func),
         offsetof(mz_gpu_window_func, width),
         offsetof(mz_gpu_window_func, nullable),
         offsetof(mz_gpu_window_func, frame),
         offsetof(mz_gpu_window_func, off),
         offsetof(mz_gpu_window_func, has_default),
         offsetof(mz_gpu_window_func, pad),
         offsetof(mz_gpu_window_func, bounds),
         offsetof(mz_gpu_window_func, offset),
         offsetof(mz_gpu_window_func, pad2),
         offsetof(mz_gpu_window_func, end_offset),
         offsetof(mz_gpu_window_func, dflt));
  printf("alias %d %u\n", f.pad, f.pad2);
  printf("consts %d %d %d %d %d %d %d %d %d %d %d %d %d\n",
         MZ_GPU_MAX_WFUNCS, MZ_WF_SUM, MZ_WF_COUNT, MZ_WF_MIN, MZ_WF_MAX,
         MZ_WF_FRAME_TO_CURRENT, MZ_WF_FRAME_PARTITION, MZ_WF_FRAME_ROWS,
         MZ_WB_UNBOUNDED_PRECEDING, MZ_WB_PRECEDING, MZ_WB_CURRENT_ROW,
         MZ_WB_FOLLOWING, MZ_WB_UNBOUNDED_FOLLOWING);
  return 0;
}
"""


def test_ctypes_mirrors_match_the_header(tmp_path):
    cc = compiler(("cc", "gcc", "clang"))
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
    alias = [int(x) for x in lines[1].split()[1:]]
    consts = [int(x) for x in lines[2].split()[1:]]
    W = abi.WindowFunc
    assert func == [abi.C.sizeof(W), W.func.offset, W.width.offset,
                    W.nullable.offset, W.frame.offset, W.off.offset,
                    W.has_default.offset, W.pad.offset, W.bounds.offset,
                    W.offset.offset, W.pad2.offset, W.end_offset.offset,
                    W.dflt.offset]
    assert func[0] == 24
    assert W.pad.offset == W.bounds.offset == 7
    assert W.pad2.offset == W.end_offset.offset == 12
    assert alias == [0x42, 7]
    assert consts == [abi.MZ_GPU_MAX_WFUNCS, abi.MZ_WF_SUM, abi.MZ_WF_COUNT,
                      abi.MZ_WF_MIN, abi.MZ_WF_MAX,
                      abi.MZ_WF_FRAME_TO_CURRENT, abi.MZ_WF_FRAME_PARTITION,
                      abi.MZ_WF_FRAME_ROWS, abi.MZ_WB_UNBOUNDED_PRECEDING,
                      abi.MZ_WB_PRECEDING, abi.MZ_WB_CURRENT_ROW,
                      abi.MZ_WB_FOLLOWING, abi.MZ_WB_UNBOUNDED_FOLLOWING]


def test_c_layer_spec_checker(tmp_path):
    """csrc/window_spec_check.cpp: window_spec_error, the C layer's own
    statement of the rules above, over the same refusals and legal edges,
    as a stand-alone host program (the Makefile's window-spec-check target
    builds the same file under the address and undefined-behaviour
    sanitizers)."""
    cxx = compiler(("c++", "g++", "clang++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "window_spec_check"
    subprocess.run([cxx, "-std=c++17", "-Wall", os.path.join(
        REPO, "materialize_amd", "csrc", "window_spec_check.cpp"), "-o",
        str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "window_spec_check: ok" in run.stdout
