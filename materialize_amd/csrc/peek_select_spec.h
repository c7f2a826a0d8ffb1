// The call-time rules of mz_gpu_peek_select (include/mz_gpu.h, "Errors")
// about its key range and its finishing, and the small host computations
// the finishing needs. Plain C++ that needs no HIP, so that
// peek_select_check.cpp can run them under the host sanitizers; mzgpu.hip
// includes it. _abi.py's peek_select_error states the same rules with the
// same messages.
#ifndef MZ_PEEK_SELECT_SPEC_H
#define MZ_PEEK_SELECT_SPEC_H

#include "../../include/mz_gpu.h"

#include <cstdint>
#include <string>

// The range rules for an arrangement of kw key words; "" when acceptable.
static inline std::string peek_range_error(const mz_gpu_key_range *r,
                                           uint32_t kw) {
  const std::string w = "peek_select: range: ";
  if (r->lo_kind > MZ_KB_EXCLUSIVE || r->hi_kind > MZ_KB_EXCLUSIVE)
    return w + "unknown bound kind " +
           std::to_string(r->lo_kind > MZ_KB_EXCLUSIVE ? r->lo_kind
                                                       : r->hi_kind);
  for (uint32_t i = 0; i < 2; i++) {
    if (i >= kw && (r->lo[i] || r->hi[i]))
      return w + "nonzero bound word beyond key_words";
    if ((r->lo_kind == MZ_KB_UNBOUNDED && r->lo[i]) ||
        (r->hi_kind == MZ_KB_UNBOUNDED && r->hi[i]))
      return w + "nonzero bound word on an unbounded side";
  }
  return "";
}

// The finishing rules against the out row it orders (okw key words, ovb val
// bytes: the mfp's out schema, or the arrangement's without an mfp); ""
// when acceptable.
static inline std::string peek_finishing_error(const mz_gpu_finishing *f,
                                               uint32_t okw, uint32_t ovb,
                                               int allow_negative) {
  const std::string p = "peek_select: ";
  if (f->n_order > MZ_GPU_MAX_ORDER)
    return p + "n_order must be at most " + std::to_string(MZ_GPU_MAX_ORDER);
  for (uint32_t j = 0; j < f->n_order; j++) {
    const mz_gpu_peek_order &oc = f->order[j];
    const std::string who = p + "order column " + std::to_string(j);
    if (oc.src != MZ_SRC_KEY && oc.src != MZ_SRC_VAL_LOOKUP)
      return who + ": src must be MZ_SRC_KEY or MZ_SRC_VAL_LOOKUP";
    if (oc.src == MZ_SRC_KEY) {
      if (oc.width != 8) return who + ": a key column must be width 8";
      if (oc.off % 8 || oc.off >= 8u * okw)
        return who + ": a key column must sit at a word boundary inside the "
                     "out key";
      if (oc.null_off != MZ_GPU_NO_NULL)
        return who + ": a key column takes no null_off";
    } else {
      if (oc.width != 4 && oc.width != 8 && oc.width != 16)
        return who + ": width must be 4, 8 or 16";
      if ((uint32_t)oc.off + oc.width > ovb)
        return who + " reads past the out val";
      if (oc.null_off != MZ_GPU_NO_NULL) {
        if (oc.null_off >= ovb) return who + ": null_off is past the out val";
        if (oc.null_off >= oc.off &&
            (uint32_t)oc.null_off < (uint32_t)oc.off + oc.width)
          return who + ": null_off is inside its own datum";
      }
    }
    if (oc.desc > 1 || oc.nulls_last > 1)
      return who + ": desc and nulls_last must be 0 or 1";
  }
  if (allow_negative)
    return p + "a finishing cannot be combined with allow_negative";
  return "";
}

// Is a finishing the identity (n_order == 0, offset == 0, no limit)?
static inline bool peek_finishing_is_identity(const mz_gpu_finishing *f) {
  return f->n_order == 0 && f->offset == 0 && f->limit < 0;
}

// End of the kept position window [offset, end): offset + limit without
// wrapping, or UINT64_MAX for no limit (positions stay below 2^63).
static inline uint64_t peek_window_end(uint64_t offset, int64_t limit) {
  if (limit < 0) return UINT64_MAX;
  const uint64_t l = (uint64_t)limit;
  return offset > UINT64_MAX - l ? UINT64_MAX : offset + l;
}

// The exact total multiplicity from the sums of the counts' high and low 32
// bits (each sum is exact in a u64 for fewer than 2^32 rows of positive
// i64 counts). Returns false when the total exceeds INT64_MAX.
static inline bool peek_total_fits(uint64_t hi_sum, uint64_t lo_sum,
                                   uint64_t *total) {
  // total = hi_sum * 2^32 + lo_sum <= INT64_MAX
  if (hi_sum >> 31) return false;  // hi_sum * 2^32 alone is >= 2^63
  const uint64_t h = hi_sum << 32;
  if (lo_sum > (uint64_t)INT64_MAX - h) return false;
  *total = h + lo_sum;
  return true;
}

#endif  // MZ_PEEK_SELECT_SPEC_H
