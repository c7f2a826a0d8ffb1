// Stand-alone check of mz_gpu_peek_select's call-time rules
// (peek_select_spec.h) for the host sanitizers: every refused and every
// edge-legal range and finishing of include/mz_gpu.h goes through
// peek_range_error / peek_finishing_error and the message is compared; the
// window end and the exact-total helpers are checked at their edges. Runs
// on the CPU; `make peek-select-check`.
#include "peek_select_spec.h"

#include <cstdio>
#include <cstring>
#include <string>

static int failures = 0;

static void expect(const char *what, const std::string &got,
                   const char *want) {
  const bool ok = *want ? got.find(want) != std::string::npos : got.empty();
  if (!ok) {
    std::printf("FAIL %s: got \"%s\", want \"%s\"\n", what, got.c_str(),
                want);
    failures++;
  }
}

static void expect_true(const char *what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    failures++;
  }
}

static mz_gpu_key_range range(uint8_t lk, int64_t lo0, int64_t lo1,
                              uint8_t hk, int64_t hi0, int64_t hi1) {
  mz_gpu_key_range r;
  std::memset(&r, 0, sizeof(r));
  r.lo_kind = lk;
  r.hi_kind = hk;
  r.lo[0] = lo0;
  r.lo[1] = lo1;
  r.hi[0] = hi0;
  r.hi[1] = hi1;
  return r;
}

static mz_gpu_peek_order col(uint8_t src, uint16_t off, uint8_t width = 8,
                             uint16_t null_off = MZ_GPU_NO_NULL,
                             uint8_t desc = 0, uint8_t nulls_last = 0) {
  mz_gpu_peek_order o;
  std::memset(&o, 0, sizeof(o));
  o.src = src;
  o.off = off;
  o.width = width;
  o.null_off = null_off;
  o.desc = desc;
  o.nulls_last = nulls_last;
  return o;
}

// out row: okw key words, ovb val bytes
static std::string fin(uint32_t okw, uint32_t ovb,
                       std::initializer_list<mz_gpu_peek_order> cols,
                       int allow_negative = 0) {
  mz_gpu_finishing f;
  std::memset(&f, 0, sizeof(f));
  f.limit = -1;
  for (const mz_gpu_peek_order &c : cols) {
    if (f.n_order < MZ_GPU_MAX_ORDER) f.order[f.n_order] = c;
    f.n_order++;
  }
  return peek_finishing_error(&f, okw, ovb, allow_negative);
}

int main() {
  const uint8_t U = MZ_KB_UNBOUNDED, I = MZ_KB_INCLUSIVE,
                X = MZ_KB_EXCLUSIVE;
  const uint8_t K = MZ_SRC_KEY, V = MZ_SRC_VAL_LOOKUP;
  mz_gpu_key_range r;

  // ranges
  r = range(3, 0, 0, I, 5, 0);
  expect("lo kind 3", peek_range_error(&r, 1),
         "peek_select: range: unknown bound kind 3");
  r = range(I, 0, 0, 255, 5, 0);
  expect("hi kind 255", peek_range_error(&r, 1), "unknown bound kind 255");
  r = range(I, 1, 7, I, 5, 0);
  expect("lo word beyond kw", peek_range_error(&r, 1),
         "nonzero bound word beyond key_words");
  r = range(I, 1, 0, X, 5, -1);
  expect("hi word beyond kw", peek_range_error(&r, 1),
         "nonzero bound word beyond key_words");
  r = range(U, 1, 0, I, 5, 0);
  expect("unbounded lo with a word", peek_range_error(&r, 1),
         "nonzero bound word on an unbounded side");
  r = range(I, 1, 0, U, 0, 2);
  expect("unbounded hi with a word", peek_range_error(&r, 2),
         "nonzero bound word on an unbounded side");
  r = range(U, 0, 0, U, 0, 0);
  expect("both unbounded", peek_range_error(&r, 1), "");
  r = range(I, INT64_MIN, 0, X, INT64_MAX, 0);
  expect("extreme bounds", peek_range_error(&r, 1), "");
  r = range(X, 9, 0, I, -9, 0);
  expect("lo > hi is legal", peek_range_error(&r, 1), "");
  r = range(I, 1, INT64_MIN, I, 1, INT64_MAX);
  expect("two words", peek_range_error(&r, 2), "");

  // finishing: out row of 2 key words and 25 val bytes, e.g. an i32 at 0
  // and an i64 at 4 with its null byte at 12
  expect("five columns",
         fin(2, 25, {col(K, 0), col(K, 8), col(V, 0, 4), col(V, 4), col(K, 0)}),
         "peek_select: n_order must be at most 4");
  expect("src stream", fin(2, 25, {col(MZ_SRC_VAL_STREAM, 0)}),
         "order column 0: src must be MZ_SRC_KEY or MZ_SRC_VAL_LOOKUP");
  expect("src compute", fin(2, 25, {col(K, 0), col(MZ_SRC_COMPUTE, 0)}),
         "order column 1: src must be");
  expect("key width 4", fin(2, 25, {col(K, 0, 4)}),
         "a key column must be width 8");
  expect("key width 16", fin(2, 25, {col(K, 0, 16)}),
         "a key column must be width 8");
  expect("key unaligned", fin(2, 25, {col(K, 4)}),
         "a key column must sit at a word boundary inside the out key");
  expect("key past", fin(2, 25, {col(K, 16)}),
         "a key column must sit at a word boundary inside the out key");
  expect("key word 1 of 1", fin(1, 25, {col(K, 8)}),
         "word boundary inside the out key");
  expect("key null_off", fin(2, 25, {col(K, 0, 8, 0)}),
         "a key column takes no null_off");
  expect("val width 2", fin(2, 25, {col(V, 0, 2)}),
         "order column 0: width must be 4, 8 or 16");
  expect("val width 0", fin(2, 25, {col(V, 0, 0)}),
         "width must be 4, 8 or 16");
  expect("val reads past", fin(2, 25, {col(V, 18)}),
         "order column 0 reads past the out val");
  expect("val 16 reads past", fin(2, 25, {col(V, 10, 16)}),
         "reads past the out val");
  expect("val on an empty val", fin(1, 0, {col(V, 0, 4)}),
         "reads past the out val");
  expect("null_off past", fin(2, 25, {col(V, 4, 8, 25)}),
         "null_off is past the out val");
  expect("null_off inside, first byte", fin(2, 25, {col(V, 4, 8, 4)}),
         "null_off is inside its own datum");
  expect("null_off inside, last byte", fin(2, 25, {col(V, 8, 16, 23)}),
         "null_off is inside its own datum");
  expect("desc 2", fin(2, 25, {col(V, 4, 8, 12, 2)}),
         "desc and nulls_last must be 0 or 1");
  expect("nulls_last 2", fin(2, 25, {col(K, 8, 8, MZ_GPU_NO_NULL, 1, 2)}),
         "desc and nulls_last must be 0 or 1");
  expect("allow_negative", fin(2, 25, {}, 1),
         "peek_select: a finishing cannot be combined with allow_negative");

  // legal edges
  expect("no columns", fin(1, 0, {}), "");
  expect("last key word", fin(2, 0, {col(K, 8, 8, MZ_GPU_NO_NULL, 1, 1)}), "");
  expect("null byte after the datum", fin(1, 25, {col(V, 4, 8, 12)}), "");
  expect("null byte before the datum (a reduce slot)",
         fin(2, 24, {col(V, 8, 16, 0, 1)}), "");
  expect("last val bytes", fin(1, 25, {col(V, 21, 4), col(V, 9, 16, 8)}), "");
  expect("null byte is the last val byte", fin(1, 25, {col(V, 0, 4, 24)}),
         "");
  expect("four columns",
         fin(2, 25, {col(K, 0), col(K, 8), col(V, 0, 4), col(V, 4)}), "");

  // identity, window end, exact total
  {
    mz_gpu_finishing f;
    std::memset(&f, 0, sizeof(f));
    f.limit = -1;
    expect_true("identity", peek_finishing_is_identity(&f));
    f.limit = 0;
    expect_true("limit 0 is not", !peek_finishing_is_identity(&f));
    f.limit = -1;
    f.offset = 1;
    expect_true("offset is not", !peek_finishing_is_identity(&f));
    f.offset = 0;
    f.n_order = 1;
    expect_true("an order is not", !peek_finishing_is_identity(&f));
  }
  expect_true("end: no limit", peek_window_end(5, -1) == UINT64_MAX);
  expect_true("end: plain", peek_window_end(5, 10) == 15);
  expect_true("end: limit 0", peek_window_end(5, 0) == 5);
  expect_true("end: saturates",
              peek_window_end(UINT64_MAX - 1, INT64_MAX) == UINT64_MAX);
  expect_true("end: exact at the top",
              peek_window_end(UINT64_MAX - 7, 7) == UINT64_MAX);
  {
    uint64_t t = 0;
    // 2^62 + (2^62 - 1): hi parts 2^30 + (2^30 - 1), lo parts 0 + (2^32 - 1)
    expect_true("total 2^63 - 1 fits",
                peek_total_fits((1ull << 30) + (1ull << 30) - 1,
                                0xFFFFFFFFull, &t) &&
                    t == (uint64_t)INT64_MAX);
    expect_true("total 2^63 does not", !peek_total_fits(1ull << 31, 0, &t));
    expect_true("carry out of the low sum",
                !peek_total_fits((1ull << 31) - 1, 1ull << 32, &t));
    expect_true("three times 2^62", !peek_total_fits(3ull << 30, 0, &t));
    expect_true("huge high sum", !peek_total_fits(UINT64_MAX, UINT64_MAX, &t));
    expect_true("low sum above 2^32",
                peek_total_fits(1, 5ull << 32, &t) && t == (6ull << 32));
    expect_true("zero", peek_total_fits(0, 0, &t) && t == 0);
  }
  std::printf(failures ? "peek_select_check: %d failures\n"
                       : "peek_select_check: ok\n",
              failures);
  return failures ? 1 : 0;
}
