// The window operator's create-time rules (include/mz_gpu.h, "Refused at
// create") and the small predicates about its functions. Plain C++ that
// needs no HIP, so that window_spec_check.cpp can run the rules under the
// host sanitizers; mzgpu.hip includes it and its kernels share the
// predicates. _abi.py's window_spec states the same rules with the same
// messages.
#ifndef MZ_WINDOW_SPEC_H
#define MZ_WINDOW_SPEC_H

#include "../../include/mz_gpu.h"

#include <cstdint>
#include <string>

#define WIN_MAX_OVB 64

// the predicates are shared with the emit kernel
#ifdef __HIPCC__
#define MZ_WF_HD __host__ __device__
#else
#define MZ_WF_HD
#endif

MZ_WF_HD static inline bool wf_is_agg(uint8_t func) {
  return func >= MZ_WF_SUM && func <= MZ_WF_MAX;
}
// LAG / LEAD / FIRST_VALUE / LAST_VALUE / SUM / MIN / MAX: a 9-byte value
// slot; the ranks and COUNT fill an i64.
MZ_WF_HD static inline bool wf_is_value(uint8_t func) {
  return func >= MZ_WF_LAG && func != MZ_WF_COUNT;
}
MZ_WF_HD static inline uint32_t wf_slot_bytes(uint8_t func) {
  return wf_is_value(func) ? 9 : 8;
}
MZ_WF_HD static inline uint32_t wf_start_kind(const mz_gpu_window_func &fn) {
  return fn.bounds & 15u;
}
MZ_WF_HD static inline uint32_t wf_end_kind(const mz_gpu_window_func &fn) {
  return fn.bounds >> 4;
}
// ROWS with both ends unbounded is the whole partition.
MZ_WF_HD static inline bool wf_rows_whole(const mz_gpu_window_func &fn) {
  return wf_start_kind(fn) == MZ_WB_UNBOUNDED_PRECEDING &&
         wf_end_kind(fn) == MZ_WB_UNBOUNDED_FOLLOWING;
}
// Does the function's value differ between the copies of one row?
MZ_WF_HD static inline bool wf_expands(const mz_gpu_window_func &fn) {
  if (wf_is_agg(fn.func))
    return fn.frame == MZ_WF_FRAME_ROWS && !wf_rows_whole(fn);
  return fn.func == MZ_WF_ROW_NUMBER || fn.func == MZ_WF_LAG ||
         fn.func == MZ_WF_LEAD;
}

// An aggregate's frame, datum and unused fields; "" when acceptable.
static inline std::string window_agg_error(const mz_gpu_window_func &fn,
                                           uint32_t vb,
                                           const std::string &who) {
  if (fn.frame > MZ_WF_FRAME_ROWS)
    return who + ": unknown frame " + std::to_string(fn.frame);
  const bool star = fn.func == MZ_WF_COUNT && fn.width == 0;
  if (!star && fn.width != 4 && fn.width != 8)
    return who + ": datum width must be 4 or 8" +
           (fn.func == MZ_WF_COUNT ? ", or 0 for COUNT(*)" : "");
  if (star && (fn.off || fn.nullable))
    return who + ": COUNT(*) takes no datum";
  if (!star && (uint32_t)fn.off + fn.width + (fn.nullable ? 1u : 0u) > vb)
    return who + " reads past in.val_bytes";
  if (fn.has_default || fn.dflt)
    return who + ": an aggregate takes no default";
  if (fn.frame != MZ_WF_FRAME_ROWS) {
    if (fn.bounds || fn.offset || fn.end_offset)
      return who + ": bounds and offsets need MZ_WF_FRAME_ROWS";
    return "";
  }
  const uint32_t sk = wf_start_kind(fn), ek = wf_end_kind(fn);
  if (sk > MZ_WB_UNBOUNDED_FOLLOWING || ek > MZ_WB_UNBOUNDED_FOLLOWING)
    return who + ": unknown bound kind " +
           std::to_string(sk > MZ_WB_UNBOUNDED_FOLLOWING ? sk : ek);
  if (sk == MZ_WB_UNBOUNDED_FOLLOWING)
    return who + ": a frame cannot start at UNBOUNDED FOLLOWING";
  if (ek == MZ_WB_UNBOUNDED_PRECEDING)
    return who + ": a frame cannot end at UNBOUNDED PRECEDING";
  if (sk == MZ_WB_CURRENT_ROW && ek == MZ_WB_PRECEDING)
    return who + ": a frame starting at CURRENT ROW cannot end PRECEDING";
  if (sk == MZ_WB_FOLLOWING &&
      (ek == MZ_WB_PRECEDING || ek == MZ_WB_CURRENT_ROW))
    return who +
           ": a frame starting FOLLOWING cannot end PRECEDING or at "
           "CURRENT ROW";
  if ((fn.offset && sk != MZ_WB_PRECEDING && sk != MZ_WB_FOLLOWING) ||
      (fn.end_offset && ek != MZ_WB_PRECEDING && ek != MZ_WB_FOLLOWING))
    return who + ": an offset on an UNBOUNDED or CURRENT ROW bound";
  if ((fn.func == MZ_WF_MIN || fn.func == MZ_WF_MAX) &&
      sk != MZ_WB_UNBOUNDED_PRECEDING && ek != MZ_WB_UNBOUNDED_FOLLOWING)
    return who +
           ": MIN / MAX over a ROWS frame bounded on both sides is not "
           "provided (it needs a range-minimum structure)";
  return "";
}

// The create-time rules of mz_gpu.h; "" when the spec is acceptable.
static inline std::string window_spec_error(const mz_gpu_window_spec *sp) {
  const uint32_t vb = sp->in.val_bytes;
  if (vb == 0xFFFFFFFFu || sp->out.val_bytes == 0xFFFFFFFFu)
    return "varlen vals unsupported";
  if (sp->in.key_words < 1 || sp->in.key_words > 2)
    return "key_words must be 1 or 2";
  if (sp->n_funcs < 1 || sp->n_funcs > MZ_GPU_MAX_WFUNCS)
    return "n_funcs must be 1.." + std::to_string(MZ_GPU_MAX_WFUNCS);
  if (sp->n_order > MZ_GPU_MAX_ORDER)
    return "n_order must be at most " + std::to_string(MZ_GPU_MAX_ORDER);
  for (uint32_t j = 0; j < sp->n_order; j++) {
    const mz_gpu_order_col &oc = sp->order[j];
    std::string who = "order column " + std::to_string(j);
    if (oc.width != 4 && oc.width != 8) return who + ": width must be 4 or 8";
    if ((uint32_t)oc.off + oc.width > vb)
      return who + " reads past in.val_bytes";
  }
  uint64_t ovb = vb;
  for (uint32_t f = 0; f < sp->n_funcs; f++) {
    const mz_gpu_window_func &fn = sp->funcs[f];
    std::string who = "func " + std::to_string(f);
    if (wf_is_agg(fn.func)) {
      std::string why = window_agg_error(fn, vb, who);
      if (!why.empty()) return why;
    } else {
      if (fn.func > MZ_WF_LAST_VALUE)
        return who + ": unknown func " + std::to_string(fn.func);
      // MZ_WF_FRAME_ROWS is the aggregates' alone
      if (fn.frame > MZ_WF_FRAME_ROWS ||
          (fn.frame > MZ_WF_FRAME_PARTITION && fn.func == MZ_WF_LAST_VALUE))
        return who + ": unknown frame " + std::to_string(fn.frame);
      if (fn.frame && fn.func != MZ_WF_LAST_VALUE)
        return who + ": a frame is for LAST_VALUE only";
      if (wf_is_value(fn.func)) {
        if (fn.width != 4 && fn.width != 8)
          return who + ": datum width must be 4 or 8";
        if ((uint32_t)fn.off + fn.width + (fn.nullable ? 1u : 0u) > vb)
          return who + " reads past in.val_bytes";
      }
    }
    ovb += wf_slot_bytes(fn.func);
  }
  if (ovb > WIN_MAX_OVB)
    return "out val is " + std::to_string(ovb) + " bytes, more than " +
           std::to_string(WIN_MAX_OVB);
  if (sp->out.key_words != sp->in.key_words || sp->out.val_bytes != ovb)
    return "out schema must be in.key_words key words and " +
           std::to_string(ovb) + " val bytes (in val ++ slots)";
  return "";
}

#endif  // MZ_WINDOW_SPEC_H
