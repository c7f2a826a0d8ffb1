// Stand-alone check of the window operator's create-time rules
// (window_spec.h) for the host sanitizers: every refused and every
// edge-legal spec of include/mz_gpu.h goes through window_spec_error and
// the message is compared. Runs on the CPU; `make window-spec-check`.
#include "window_spec.h"

#include <cstdio>
#include <cstring>
#include <string>

static int failures = 0;

static mz_gpu_window_func fn(uint8_t func, uint16_t off = 0,
                             uint8_t width = 0, uint8_t nullable = 0,
                             uint8_t frame = 0) {
  mz_gpu_window_func f;
  std::memset(&f, 0, sizeof(f));
  f.func = func;
  f.off = off;
  f.width = width;
  f.nullable = nullable;
  f.frame = frame;
  return f;
}

static mz_gpu_window_func rows(uint8_t func, uint32_t sk, uint32_t k,
                               uint32_t ek, uint32_t k2, uint16_t off = 8,
                               uint8_t width = 8, uint8_t nullable = 1) {
  mz_gpu_window_func f = fn(func, off, width, nullable, MZ_WF_FRAME_ROWS);
  f.bounds = (uint8_t)(sk | ek << 4);
  f.offset = k;
  f.end_offset = k2;
  return f;
}

// in: 1 key word, vb val bytes; out derived unless out_vb is given
static std::string check(uint32_t vb, std::initializer_list<mz_gpu_window_func> fs,
                         int64_t out_vb = -1) {
  mz_gpu_window_spec sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.in.key_words = 1;
  sp.in.val_bytes = vb;
  uint32_t ovb = vb;
  for (const mz_gpu_window_func &f : fs) {
    if (sp.n_funcs < MZ_GPU_MAX_WFUNCS) sp.funcs[sp.n_funcs] = f;
    sp.n_funcs++;
    ovb += wf_slot_bytes(f.func);
  }
  sp.out.key_words = 1;
  sp.out.val_bytes = out_vb < 0 ? ovb : (uint32_t)out_vb;
  return window_spec_error(&sp);
}

static void expect(const char *what, const std::string &got,
                   const char *want) {
  const bool ok = *want ? got.find(want) != std::string::npos : got.empty();
  if (!ok) {
    std::printf("FAIL %s: got \"%s\", want \"%s\"\n", what, got.c_str(),
                want);
    failures++;
  }
}

int main() {
  const uint32_t UP = MZ_WB_UNBOUNDED_PRECEDING, P = MZ_WB_PRECEDING,
                 C = MZ_WB_CURRENT_ROW, F = MZ_WB_FOLLOWING,
                 UF = MZ_WB_UNBOUNDED_FOLLOWING;
  const uint32_t VB = 17;  // a i32 @0, b i32 @4, x i64 @8 with null byte @16

  // funcs 0..6: texts and order unchanged
  expect("unknown func", check(VB, {fn(7)}), "func 0: unknown func 7");
  expect("unknown func 15", check(VB, {fn(15)}), "unknown func 15");
  expect("unknown func 20", check(VB, {fn(20)}), "unknown func 20");
  expect("last_value frame 2",
         check(VB, {fn(MZ_WF_LAST_VALUE, 0, 4, 0, 2)}), "unknown frame 2");
  expect("first_value frame",
         check(VB, {fn(MZ_WF_FIRST_VALUE, 0, 4, 0, 1)}), "LAST_VALUE only");
  expect("rank ROWS", check(VB, {fn(MZ_WF_RANK, 0, 0, 0, 2)}),
         "LAST_VALUE only");
  expect("lag ROWS", check(VB, {fn(MZ_WF_LAG, 0, 4, 0, 2)}),
         "LAST_VALUE only");
  expect("rank frame 3", check(VB, {fn(MZ_WF_RANK, 0, 0, 0, 3)}),
         "unknown frame 3");
  expect("lag width", check(VB, {fn(MZ_WF_LAG, 0, 2)}), "datum width");
  expect("first_value past",
         check(VB, {fn(MZ_WF_RANK), fn(MZ_WF_FIRST_VALUE, 12, 8)}),
         "func 1 reads past");

  // aggregates
  expect("sum frame 3", check(VB, {fn(MZ_WF_SUM, 8, 8, 1, 3)}),
         "func 0: unknown frame 3");
  expect("sum width 0", check(VB, {fn(MZ_WF_SUM, 8, 0)}),
         "datum width must be 4 or 8");
  expect("min width 2", check(VB, {fn(MZ_WF_MIN, 8, 2)}),
         "datum width must be 4 or 8");
  expect("count width 2", check(VB, {fn(MZ_WF_COUNT, 8, 2)}),
         "datum width must be 4 or 8, or 0 for COUNT(*)");
  expect("count(*) with off", check(VB, {fn(MZ_WF_COUNT, 8, 0)}),
         "COUNT(*) takes no datum");
  expect("sum past", check(VB, {fn(MZ_WF_SUM, 12, 8)}), "func 0 reads past");
  expect("max null byte past", check(16, {fn(MZ_WF_MAX, 8, 8, 1)}),
         "func 0 reads past");
  {
    mz_gpu_window_func f = fn(MZ_WF_SUM, 8, 8, 1);
    f.has_default = 1;
    expect("has_default", check(VB, {f}), "an aggregate takes no default");
    f.has_default = 0;
    f.dflt = -1;
    expect("dflt", check(VB, {f}), "an aggregate takes no default");
    f.dflt = 0;
    f.bounds = (uint8_t)(C | UF << 4);
    expect("bounds without ROWS", check(VB, {f}),
           "bounds and offsets need MZ_WF_FRAME_ROWS");
    f.bounds = 0;
    f.offset = 1;
    expect("offset without ROWS", check(VB, {f}),
           "bounds and offsets need MZ_WF_FRAME_ROWS");
    f.offset = 0;
    f.end_offset = 1;
    f.frame = MZ_WF_FRAME_PARTITION;
    expect("end_offset without ROWS", check(VB, {f}),
           "bounds and offsets need MZ_WF_FRAME_ROWS");
  }
  expect("start kind 5", check(VB, {rows(MZ_WF_SUM, 5, 0, C, 0)}),
         "unknown bound kind 5");
  expect("end kind 15", check(VB, {rows(MZ_WF_SUM, C, 0, 15, 0)}),
         "unknown bound kind 15");
  expect("start UF", check(VB, {rows(MZ_WF_SUM, UF, 0, UF, 0)}),
         "cannot start at UNBOUNDED FOLLOWING");
  expect("end UP", check(VB, {rows(MZ_WF_SUM, UP, 0, UP, 0)}),
         "cannot end at UNBOUNDED PRECEDING");
  expect("C..P", check(VB, {rows(MZ_WF_COUNT, C, 0, P, 1)}),
         "starting at CURRENT ROW cannot end PRECEDING");
  expect("F..P", check(VB, {rows(MZ_WF_SUM, F, 1, P, 1)}),
         "starting FOLLOWING cannot end PRECEDING or at CURRENT ROW");
  expect("F..C", check(VB, {rows(MZ_WF_SUM, F, 1, C, 0)}),
         "starting FOLLOWING cannot end PRECEDING or at CURRENT ROW");
  expect("offset on CURRENT ROW", check(VB, {rows(MZ_WF_SUM, C, 2, UF, 0)}),
         "an offset on an UNBOUNDED or CURRENT ROW bound");
  expect("offset on UNBOUNDED", check(VB, {rows(MZ_WF_SUM, UP, 0, UF, 2)}),
         "an offset on an UNBOUNDED or CURRENT ROW bound");
  expect("min two-sided", check(VB, {rows(MZ_WF_MIN, P, 1, F, 1)}),
         "bounded on both sides is not provided");
  expect("max two-sided", check(VB, {rows(MZ_WF_MAX, C, 0, C, 0)}),
         "range-minimum structure");
  expect("out too wide",
         check(40, {fn(MZ_WF_SUM, 0, 8), fn(MZ_WF_SUM, 0, 8),
                    fn(MZ_WF_SUM, 0, 8)}),
         "more than 64");
  expect("out mismatch", check(VB, {fn(MZ_WF_COUNT)}, 26),
         "out schema must be in.key_words key words and 25 val bytes");
  expect("five funcs",
         check(VB, {fn(MZ_WF_COUNT), fn(MZ_WF_COUNT), fn(MZ_WF_COUNT),
                    fn(MZ_WF_COUNT), fn(MZ_WF_COUNT)}),
         "n_funcs must be 1..4");

  // legal edges
  expect("count(*)", check(0, {fn(MZ_WF_COUNT)}), "");
  expect("count(x)", check(VB, {fn(MZ_WF_COUNT, 8, 8, 1)}), "");
  expect("64 out bytes",
         check(37, {fn(MZ_WF_SUM, 28, 8, 1), fn(MZ_WF_MIN, 28, 8, 1),
                    fn(MZ_WF_MAX, 28, 8, 1)}),
         "");
  expect("3 PRECEDING .. 5 PRECEDING",
         check(VB, {rows(MZ_WF_SUM, P, 3, P, 5)}), "");
  expect("both unbounded", check(VB, {rows(MZ_WF_MIN, UP, 0, UF, 0)}), "");
  expect("min UP..k F", check(VB, {rows(MZ_WF_MIN, UP, 0, F, 2)}), "");
  expect("max k P..UF", check(VB, {rows(MZ_WF_MAX, P, 2, UF, 0)}), "");
  expect("partition sum", check(VB, {fn(MZ_WF_SUM, 0, 4, 0, 1)}), "");
  expect("mixed",
         check(VB, {fn(MZ_WF_ROW_NUMBER), rows(MZ_WF_SUM, P, 1, F, 1),
                    fn(MZ_WF_LAG, 8, 8, 1), fn(MZ_WF_COUNT)}),
         "");
  {
    mz_gpu_window_func a = rows(MZ_WF_SUM, UP, 0, UF, 0);
    mz_gpu_window_func b = rows(MZ_WF_SUM, UP, 0, C, 0);
    if (wf_expands(a) || !wf_expands(b) ||
        wf_expands(fn(MZ_WF_SUM, 8, 8, 1, MZ_WF_FRAME_PARTITION)) ||
        !wf_expands(fn(MZ_WF_LEAD, 8, 8)) || wf_expands(fn(MZ_WF_RANK))) {
      std::printf("FAIL wf_expands\n");
      failures++;
    }
  }
  if (wf_slot_bytes(MZ_WF_COUNT) != 8 || wf_slot_bytes(MZ_WF_SUM) != 9 ||
      wf_slot_bytes(MZ_WF_MIN) != 9 || wf_slot_bytes(MZ_WF_MAX) != 9 ||
      wf_slot_bytes(MZ_WF_RANK) != 8 || wf_slot_bytes(MZ_WF_LAG) != 9) {
    std::printf("FAIL wf_slot_bytes\n");
    failures++;
  }
  std::printf(failures ? "window_spec_check: %d failures\n"
                       : "window_spec_check: ok\n",
              failures);
  return failures ? 1 : 0;
}
