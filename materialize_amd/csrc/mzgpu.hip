// mzgpu.hip — MI355X-native incremental join/reduce engine (PRODUCT).
//
// Implements the C ABI of include/mz_gpu.h with hand-written HIP kernels
// for gfx950. All hot work is HBM-bound integer/byte processing (hash
// probes, sort-based consolidation, segmented accumulation) — no MFMA.
// Sort/scan primitives come from rocPRIM (AMD-native); the probe,
// consolidate-emit, batch-build, hash and reduce kernels are hand-written.
//
// Replaces (reference file:line under /root/reference — algorithms
// restated, not translated):
//   mz_join_core            src/compute/src/render/join/mz_join_core.rs:57-496
//   half_join stages        src/compute/src/render/join/delta_join.rs:338-583
//   build_accumulable       src/compute/src/render/reduce.rs:1357-1581,1611-2270
//   arrangement/spine       src/compute/src/extensions/arrange.rs:69-114,
//                           src/row-spine/src/lib.rs:56-135
//   Exchange routing        src/compute/src/render/join/linear_join.rs:390
//
// The cross-product ("simple") join strategy is applied at update
// granularity; after consolidation its results are identical to the
// reference's EditList/linear-scan pipeline (bilinearity — DESIGN.md §5),
// which the oracle (which implements both strategies) verifies.

#include "common.h"
#include "../../include/mz_gpu.h"
#include "peek_select_spec.h"
#include "window_spec.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

// ------------------------------------------------------------------ utils

static constexpr int BLK = 256;
static inline u32 ngrid(u64 n) {
  u64 g = (n + BLK - 1) / BLK;
  return (u32)std::min<u64>(g, 8 * 256);  // cap; kernels grid-stride
}
#define GRID_STRIDE(i, n)                                     \
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < (n); \
       i += (u64)gridDim.x * blockDim.x)

__device__ __forceinline__ i64 wadd(i64 a, i64 b) {
  return (i64)((u64)a + (u64)b);
}
__device__ __forceinline__ i64 wmul(i64 a, i64 b) {
  return (i64)((u64)a * (u64)b);
}

// ------------------------------------------------- elementary kernels

__global__ void k_iota(u32 *p, u64 n) { GRID_STRIDE(i, n) p[i] = (u32)i; }

__global__ void k_iota_off(u32 *p, u64 n, u32 base) {
  GRID_STRIDE(i, n) p[i] = base + (u32)i;
}

__global__ void k_gather_u64(const u64 *src, const u32 *perm, u64 *dst,
                             u64 n) {
  GRID_STRIDE(i, n) dst[i] = src[perm[i]];
}
__global__ void k_gather_i64(const i64 *src, const u32 *perm, i64 *dst,
                             u64 n) {
  GRID_STRIDE(i, n) dst[i] = src[perm[i]];
}
__global__ void k_gather_keyrows(const u64 *src, u32 kw, const u32 *perm,
                                 u64 *dst, u64 n) {
  GRID_STRIDE(i, n) {
    for (u32 w = 0; w < kw; w++) dst[i * kw + w] = src[(u64)perm[i] * kw + w];
  }
}
__global__ void k_gather_valrows(const u8 *src, u32 vb, const u32 *perm,
                                 u8 *dst, u64 n) {
  GRID_STRIDE(i, n) {
    const u8 *s = src + (u64)perm[i] * vb;
    u8 *d = dst + i * vb;
    for (u32 b = 0; b < vb; b++) d[b] = s[b];
  }
}

// all four columns of an update stream at once (vb == 0: no val column)
__global__ void k_gather_updates(const u64 *keys, u32 kw, const u8 *vals,
                                 u32 vb, const u64 *times, const i64 *diffs,
                                 const u32 *perm, u64 *okeys, u8 *ovals,
                                 u64 *otimes, i64 *odiffs, u64 n) {
  GRID_STRIDE(i, n) {
    u64 r = perm[i];
    for (u32 w = 0; w < kw; w++) okeys[i * kw + w] = keys[r * kw + w];
    for (u32 b = 0; b < vb; b++) ovals[i * vb + b] = vals[r * vb + b];
    otimes[i] = times[r];
    odiffs[i] = diffs[r];
  }
}

// Two update streams of n1 and n2 rows laid end to end, in one launch.
__global__ void k_concat_updates(const u64 *k1, const u8 *v1, const u64 *t1,
                                 const i64 *d1, u64 n1, const u64 *k2,
                                 const u8 *v2, const u64 *t2, const i64 *d2,
                                 u64 n2, u32 kw, u32 vb, u64 *okeys,
                                 u8 *ovals, u64 *otimes, i64 *odiffs) {
  GRID_STRIDE(i, n1 + n2) {
    bool first = i < n1;
    u64 r = first ? i : i - n1;
    const u64 *k = first ? k1 : k2;
    const u8 *v = first ? v1 : v2;
    for (u32 w = 0; w < kw; w++) okeys[i * kw + w] = k[r * kw + w];
    for (u32 b = 0; b < vb; b++) ovals[i * vb + b] = v[r * vb + b];
    otimes[i] = (first ? t1 : t2)[r];
    odiffs[i] = (first ? d1 : d2)[r];
  }
}

// The sort-key kernels read row perm[i]. The first one of a sort has no
// permutation yet: it gets `ident` instead, reads row i and writes the
// identity there, which saves a separate iota launch.
__device__ __forceinline__ u64 sort_row(const u32 *perm, u32 *ident, u64 i) {
  if (!ident) return perm[i];
  ident[i] = (u32)i;
  return i;
}

// sort key for one key word: flip sign bit -> unsigned order == i64 order
__global__ void k_sortkey_key(const u64 *keys, u32 kw, u32 word,
                              const u32 *perm, u64 *out, u64 n, u64 sub,
                              u32 *ident) {
  GRID_STRIDE(i, n)
  out[i] = (keys[sort_row(perm, ident, i) * kw + word] ^
            0x8000000000000000ULL) - sub;
}
// sort key for one 8-byte val group: zero-padded little-endian u64 word
// (the engine's canonical val order — matches oracle cmp_val)
__device__ __forceinline__ u64 le_val_word(const u8 *v, u32 rem) {
  u64 x = 0;
  if (rem >= 8) {
    memcpy(&x, v, 8);
  } else {
    for (u32 b = 0; b < rem; b++) x |= (u64)v[b] << (8 * b);
  }
  return x;
}

__global__ void k_sortkey_val(const u8 *vals, u32 vb, u32 word,
                              const u32 *perm, u64 *out, u64 n, u64 sub,
                              u32 *ident) {
  GRID_STRIDE(i, n) {
    const u8 *v = vals + sort_row(perm, ident, i) * vb + word * 8;
    out[i] = le_val_word(v, vb - word * 8) - sub;
  }
}

// per-pass min/max of all sort-key columns in one sweep (block LDS reduce
// + one atomic per block per pass) — lets the radix passes subtract the
// min and sort only the live bits.
// One slot per sort column: time + val words + key words. 16 covers the
// widest rows consolidated — 96-byte stitched aggregate rows (12 val
// words) under 2-word keys; at 12 those rows' key slots aliased the max
// half and the output came back grouped but out of canonical order.
#define MAX_PASSES 16
__global__ void k_pass_minmax(const u64 *keys, u32 kw, const u8 *vals,
                              u32 vb, const u64 *times, u64 n, u32 vwords,
                              int with_time, u64 *mins, u64 *maxs) {
  // one column per blockIdx.y: two registers per thread (the
  // dynamically-indexed per-column register arrays of the 1-D version
  // spilled to scratch and ran at 0.4 TB/s), one LDS merge + one global
  // atomic pair per block.
  u32 p = blockIdx.y;
  u32 t0 = with_time ? 1u : 0u;
  int kind;
  u32 word = 0;
  if (with_time && p == 0) {
    kind = 0;
  } else if (p < t0 + vwords) {
    kind = 1;
    word = p - t0;
  } else {
    kind = 2;
    word = p - t0 - vwords;
  }
  u64 lmin = ~0ull, lmax = 0;
  GRID_STRIDE(i, n) {
    u64 x;
    if (kind == 0)
      x = times[i];
    else if (kind == 1)
      x = le_val_word(vals + i * vb + word * 8, vb - word * 8);
    else
      x = keys[i * kw + word] ^ 0x8000000000000000ULL;
    lmin = x < lmin ? x : lmin;
    lmax = x > lmax ? x : lmax;
  }
  __shared__ u64 smin, smax;
  if (threadIdx.x == 0) {
    smin = ~0ull;
    smax = 0;
  }
  __syncthreads();
  atomicMin((unsigned long long *)&smin, lmin);
  atomicMax((unsigned long long *)&smax, lmax);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMin((unsigned long long *)&mins[p], smin);
    atomicMax((unsigned long long *)&maxs[p], smax);
  }
}
__global__ void k_sortkey_u64(const u64 *src, const u32 *perm, u64 *out,
                              u64 n, u64 sub, u32 *ident) {
  GRID_STRIDE(i, n) out[i] = src[sort_row(perm, ident, i)] - sub;
}

// Composite radix key: several narrowed columns packed into one u64
// (least-significant column at shift 0 == the LSD pass order), so one
// rocprim sort replaces up to MAX_COMP per-column passes.
#define MAX_COMP 6
struct CompSpec {
  u32 n;
  u32 kind[MAX_COMP];  // 0 = time, 1 = val word, 2 = key word
  u32 word[MAX_COMP];
  u64 sub[MAX_COMP];
  u32 shift[MAX_COMP];
};

__global__ void k_sortkey_comp(const u64 *keys, u32 kw, const u8 *vals,
                               u32 vb, const u64 *times, const u32 *perm,
                               u64 *out, u64 n, CompSpec sp, u32 *ident) {
  GRID_STRIDE(i, n) {
    u64 p = sort_row(perm, ident, i);
    u64 acc = 0;
    for (u32 c = 0; c < sp.n; c++) {
      u64 x;
      if (sp.kind[c] == 0)
        x = times[p];
      else if (sp.kind[c] == 1)
        x = le_val_word(vals + p * vb + sp.word[c] * 8, vb - sp.word[c] * 8);
      else
        x = keys[p * kw + sp.word[c]] ^ 0x8000000000000000ULL;
      acc |= (x - sp.sub[c]) << sp.shift[c];
    }
    out[i] = acc;
  }
}

__global__ void k_group_starts(const u32 *flags, const u32 *gid, u32 *starts,
                               u64 n) {
  GRID_STRIDE(i, n) if (flags[i]) starts[gid[i] - 1] = (u32)i;
}

// per-group wrapping diff sums via prefix differences; emit nonzero flags.
// G (group count) is read on-device from gid[n-1] so the host never has to
// synchronize for it; the grid is sized by the capacity n.
__global__ void k_group_sums(const u32 *starts, const u32 *gid, u64 n,
                             const u64 *diff_prefix /* inclusive, permuted */,
                             i64 *gsum, u32 *nz) {
  u64 G = n ? gid[n - 1] : 0;
  GRID_STRIDE(g, n) {
    if (g >= G) {
      nz[g] = 0;  // zero the padding so the nz scan over n is exact
      continue;
    }
    u64 lo = starts[g];
    u64 hi = (g + 1 < G) ? starts[g + 1] : n;
    u64 s = diff_prefix[hi - 1] - (lo ? diff_prefix[lo - 1] : 0);
    gsum[g] = (i64)s;
    nz[g] = s != 0;
  }
}

// ---- consolidation over a ready permutation: head flag +
// permuted diff, one segmented scan, one survivor scan, one emit.

// One scan element: the running wrapping diff sum of the row's group so
// far, and whether a group starts at or before it within the scanned span.
struct SegSum {
  u64 sum;
  u64 head;
};
// The segmented-sum operator (associative): a head on the right restarts.
struct SegSumOp {
  __host__ __device__ SegSum operator()(const SegSum &a,
                                        const SegSum &b) const {
    return b.head ? b : SegSum{a.sum + b.sum, a.head};
  }
};

// head flag over the permuted (key,val,time) order, with the row's diff
__global__ void k_head_diff(const u64 *keys, u32 kw, const u8 *vals, u32 vb,
                            const u64 *times, const i64 *diffs,
                            const u32 *perm, SegSum *hd, u64 n) {
  GRID_STRIDE(i, n) {
    u64 a = perm[i];
    bool neq = i == 0;
    if (!neq) {
      u64 b = perm[i - 1];
      for (u32 w = 0; w < kw; w++) neq |= keys[a * kw + w] != keys[b * kw + w];
      for (u32 c = 0; c < vb && !neq; c++)
        neq |= vals[a * vb + c] != vals[b * vb + c];
      if (!neq) neq = times[a] != times[b];
    }
    hd[i] = SegSum{(u64)diffs[a], neq ? 1ull : 0ull};
  }
}

// Row i survives iff it is the last of its group and the group's sum
// (complete at its last row) is non-zero; 0 for the scan's padding slot.
struct SurvivorIn {
  const SegSum *hd, *seg;
  u64 n;
  __host__ __device__ u32 operator()(u64 i) const {
    if (i >= n) return 0u;
    bool last = i + 1 == n || hd[i + 1].head;
    return last && seg[i].sum != 0 ? 1u : 0u;
  }
};

// Each surviving group's last row writes the group's output row: all rows
// of a group are equal on (key, val, time), so any of them serves. pos is
// the exclusive scan of SurvivorIn over n + 1 slots, pos[n] the total.
__global__ void k_emit_survivors(const u64 *keys, u32 kw, const u8 *vals,
                                 u32 vb, const u64 *times, const u32 *perm,
                                 SurvivorIn sv, const u32 *pos, u64 *okeys,
                                 u8 *ovals, u64 *otimes, i64 *odiffs,
                                 u64 *otimes2, i64 *odiffs2 /* or nullptr */,
                                 u64 *dcounts /* [0] = M out */) {
  u64 n = sv.n;
  if (blockIdx.x == 0 && threadIdx.x == 0) dcounts[0] = pos[n];
  GRID_STRIDE(i, n) {
    if (!sv(i)) continue;
    u64 o = pos[i];
    u64 r = perm[i];
    for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = keys[r * kw + w];
    for (u32 c = 0; c < vb; c++) ovals[o * vb + c] = vals[r * vb + c];
    otimes[o] = times[r];
    odiffs[o] = (i64)sv.seg[i].sum;
    if (otimes2) {
      otimes2[o] = times[r];
      odiffs2[o] = (i64)sv.seg[i].sum;
    }
  }
}

__global__ void k_advance_times(u64 *times, u64 n, u64 frontier) {
  GRID_STRIDE(i, n) times[i] = times[i] < frontier ? frontier : times[i];
}

// ----------------------------------------------- batch structure build

// Change flags over SEALED (already sorted) arrays, as the input of ONE
// scan: kc | vc << 32, where kc marks a row that opens a key and vc one that
// opens a (key, val). Both totals stay below 2^32, so the packed u64 sum is
// exact. The actual row count M is read on-device from dcounts[0] (set by
// k_emit_survivors); positions beyond it count nothing, so the
// capacity-sized scan stays exact.
struct ChangeFlagsIn {
  const u64 *keys;
  const u8 *vals;
  const u64 *dcounts;
  u32 kw, vb;
  __host__ __device__ u64 operator()(u64 i) const {
    if (i >= dcounts[0]) return 0;
    if (i == 0) return 1ull | 1ull << 32;
    bool kneq = false;
    for (u32 w = 0; w < kw; w++)
      kneq |= keys[i * kw + w] != keys[(i - 1) * kw + w];
    bool vneq = kneq;
    for (u32 c = 0; c < vb && !vneq; c++)
      vneq |= vals[i * vb + c] != vals[(i - 1) * vb + c];
    return (kneq ? 1ull : 0ull) | (vneq ? 1ull << 32 : 0ull);
  }
};

// ids: the inclusive scan of ChangeFlagsIn (key id low, val id high, both
// 1-based); a row opens a key / a val where its id differs from the row
// before.
__global__ void k_scatter_structure(const u64 *keys, u32 kw, const u8 *vals,
                                    u32 vb, const u64 *ids, u64 n,
                                    u64 *bkeys, u32 *kv_off, u8 *bvals,
                                    u32 *vu_off, u32 *val_key, u32 *upd_val,
                                    u64 *dcounts /* [0]=M in; [1]=nk,
                                                    [2]=nv out */) {
  u64 cap = n;
  n = dcounts[0];  // actual consolidated rows
  u64 n_keys = n ? (u32)ids[cap - 1] : 0;  // nothing counted beyond n
  u64 n_vals = n ? ids[cap - 1] >> 32 : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dcounts[1] = n_keys;
    dcounts[2] = n_vals;
  }
  GRID_STRIDE(i, n) {
    u64 id = ids[i], prev = i ? ids[i - 1] : 0;
    u32 k = (u32)id - 1, v = (u32)(id >> 32) - 1;
    upd_val[i] = v;
    if ((u32)id != (u32)prev) {
      for (u32 w = 0; w < kw; w++) bkeys[(u64)k * kw + w] = keys[i * kw + w];
      kv_off[k] = v;
      if (k == 0) kv_off[n_keys] = (u32)n_vals;
    }
    if (id >> 32 != prev >> 32) {
      for (u32 c = 0; c < vb; c++) bvals[(u64)v * vb + c] = vals[i * vb + c];
      vu_off[v] = (u32)i;
      val_key[v] = k;
      if (v == 0) vu_off[n_vals] = (u32)n;
    }
  }
}


// Compressed batch slot: [key words][range word], stride kw+1 (16 B for
// 1-word keys -> 4 slots per 64 B line). The packed val range
// kv_lo|kv_hi<<32 doubles as the occupancy sentinel (~0 is impossible:
// kv_hi > kv_lo and n_vals < 2^32), so the CAS publishes the range
// directly and no separate idx word is needed.
__global__ void k_hash_build(u64 *hash, u64 slots, const u64 *keys, u32 kw,
                             const u32 *kv_off,
                             const u64 *n_keys_p /* device word */) {
  u64 n_keys = *n_keys_p;
  GRID_STRIDE(i, n_keys) {
    u64 h = route_hash(keys + i * kw, kw) & (slots - 1);
    u64 range = (u64)kv_off[i] | ((u64)kv_off[i + 1] << 32);
    for (;;) {
      u64 *slot = hash + h * (kw + 1);
      unsigned long long got = atomicCAS((unsigned long long *)(slot + kw),
                                         ~0ull, (unsigned long long)range);
      if (got == ~0ull) {
        for (u32 w = 0; w < kw; w++) slot[w] = keys[i * kw + w];
        break;
      }
      h = (h + 1) & (slots - 1);
    }
  }
}

__device__ __forceinline__ int hash_lookup(const u64 *hash, u64 slots,
                                           const u64 *key, u32 kw,
                                           u32 sw) {
  if (slots == 0) return -1;
  u64 h = route_hash(key, kw) & (slots - 1);
  for (;;) {
    const u64 *slot = hash + h * sw;
    u64 iw = slot[kw];
    if (iw == ~0ull) return -1;
    bool eq = true;
    for (u32 w = 0; w < kw; w++) eq &= slot[w] == key[w];
    if (eq) return (int)(u32)iw;
    h = (h + 1) & (slots - 1);
  }
}

// Batch-table lookup returning the key's packed val range
// (kv_lo | kv_hi<<32) straight from the widened slot — one random line
// instead of two (no kv_off read). ~0 = miss.
__device__ __forceinline__ u64 hash_lookup_range(const u64 *hash, u64 slots,
                                                 const u64 *key, u32 kw) {
  if (slots == 0) return ~0ull;
  u64 h = route_hash(key, kw) & (slots - 1);
  for (;;) {
    const u64 *slot = hash + h * (kw + 1);
    u64 iw = slot[kw];  // packed range; ~0 = empty
    if (iw == ~0ull) return ~0ull;
    bool eq = true;
    for (u32 w = 0; w < kw; w++) eq &= slot[w] == key[w];
    if (eq) return iw;
    h = (h + 1) & (slots - 1);
  }
}

// ------------------------------------------------------- closure (device)

__device__ __forceinline__ i64 d_read_int(const u8 *p, u8 width) {
  if (width == 4) {
    int32_t v;
    memcpy(&v, p, 4);
    return v;
  }
  i64 v;
  memcpy(&v, p, 8);
  return v;
}

__device__ __forceinline__ const u8 *d_cl_src(const u64 *key, const u8 *v1,
                                              const u8 *v2, u8 src) {
  switch (src) {
    case MZ_SRC_KEY: return (const u8 *)key;
    case MZ_SRC_VAL_STREAM: return v1;
    default: return v2;
  }
}

// mirrors oracle closure_apply; v1 = input-1/stream val, v2 = input-2/lookup.
// Returns 0 = filtered out, 1 = ok, 2 = evaluation ERROR (division by
// zero) — the err branch of the could_error split, linear_join.rs:495.
__device__ int d_closure_apply(const mz_gpu_closure *cl, const u64 *key,
                               const u8 *v1, const u8 *v2, u64 *okey,
                               u8 *oval) {
  for (u32 i = 0; i < cl->n_filters; i++) {
    const mz_gpu_filter f = cl->filters[i];
    if (f.src == MZ_SRC_COMPUTE) {
      if (f.off == MZ_COMPUTE_Q17_QTYLT) {
        // 5*q*count < sum, count > 0 (Q17 correlated average; see header)
        i64 q = d_read_int(d_cl_src(key, v1, v2, f.arg0_src) + f.arg0, 8);
        const u8 *slot = d_cl_src(key, v1, v2, f.arg1_src) + f.arg1;
        i128 S;
        memcpy(&S, slot, 16);
        i64 C = d_read_int(slot + 24, 8);
        if (!(C > 0 && (i128)5 * q * C < S)) return false;
      }
      if (f.off == MZ_COMPUTE_CMP_FIELDS) {
        i64 x = d_read_int(d_cl_src(key, v1, v2, f.arg0_src) + f.arg0,
                           f.width);
        i64 y = d_read_int(d_cl_src(key, v1, v2, f.arg1_src) + f.arg1,
                           f.width);
        bool ok;
        switch (f.cmp) {
          case MZ_CMP_LT: ok = x < y; break;
          case MZ_CMP_LE: ok = x <= y; break;
          case MZ_CMP_GT: ok = x > y; break;
          case MZ_CMP_GE: ok = x >= y; break;
          case MZ_CMP_EQ: ok = x == y; break;
          default: ok = x != y; break;
        }
        if (!ok) return 0;
      }
      continue;
    }
    i64 x = d_read_int(d_cl_src(key, v1, v2, f.src) + f.off, f.width);
    bool ok;
    switch (f.cmp) {
      case MZ_CMP_LT: ok = x < f.imm; break;
      case MZ_CMP_LE: ok = x <= f.imm; break;
      case MZ_CMP_GT: ok = x > f.imm; break;
      case MZ_CMP_GE: ok = x >= f.imm; break;
      case MZ_CMP_EQ: ok = x == f.imm; break;
      default: ok = x != f.imm; break;
    }
    if (!ok) return 0;
  }
  if (!okey) {
    // count mode: fields are not materialized, but erroring computes
    // must still be CHECKED so ok/err counts match the emit phase
    for (int which = 0; which < 2; which++) {
      u32 nf = which ? cl->n_val_fields : cl->n_key_fields;
      const mz_gpu_field *fs = which ? cl->val_fields : cl->key_fields;
      for (u32 i = 0; i < nf; i++) {
        const mz_gpu_field f = fs[i];
        if (f.src == MZ_SRC_COMPUTE && f.off == MZ_COMPUTE_DIV_I64) {
          i64 b = d_read_int(d_cl_src(key, v1, v2, f.arg1_src) + f.arg1,
                             8);
          if (b == 0) return 2;
        }
      }
    }
    return 1;
  }
  for (int which = 0; which < 2; which++) {
    u32 nf = which ? cl->n_val_fields : cl->n_key_fields;
    const mz_gpu_field *fs = which ? cl->val_fields : cl->key_fields;
    u8 *dst = which ? oval : (u8 *)okey;
    for (u32 i = 0; i < nf; i++) {
      const mz_gpu_field f = fs[i];
      if (f.src == MZ_SRC_COMPUTE) {
        i64 v = 0;
        if (f.off == MZ_COMPUTE_REVENUE) {
          i64 ep = d_read_int(d_cl_src(key, v1, v2, f.arg0_src) + f.arg0, 8);
          i64 disc = d_read_int(d_cl_src(key, v1, v2, f.arg1_src) + f.arg1, 8);
          v = ep * (10000 - disc);
        } else if (f.off == MZ_COMPUTE_DIV_I64) {
          i64 a = d_read_int(d_cl_src(key, v1, v2, f.arg0_src) + f.arg0, 8);
          i64 b = d_read_int(d_cl_src(key, v1, v2, f.arg1_src) + f.arg1, 8);
          if (b == 0) return 2;  // -> error stream
          v = a / b;
        } else if (f.off == MZ_COMPUTE_MUL_I64) {
          i64 a = d_read_int(d_cl_src(key, v1, v2, f.arg0_src) + f.arg0, 8);
          i64 b = d_read_int(d_cl_src(key, v1, v2, f.arg1_src) + f.arg1, 8);
          v = wmul(a, b);
        }
        memcpy(dst, &v, 8);
        dst += 8;
      } else {
        const u8 *s = d_cl_src(key, v1, v2, f.src) + f.off;
        for (u32 b = 0; b < f.width; b++) dst[b] = s[b];
        dst += f.width;
      }
    }
  }
  return 1;
}

// --------------------------------------------------------------- probe

// A probe target list (snapshot of an arrangement's batches).
// allpass[i]: every update time in batch i is strictly below the delta's
// lower bound, so le/lt time filters are vacuously true and the output
// time is the stream time — the batch's time column is never read.
struct BatchList {
  int n;
  DevBatch b[12];
  u8 allpass[12];
};

enum ProbeMode { PM_JOIN = 0, PM_HALF_LE = 1, PM_HALF_LT = 2 };

// The delta stream as every probe kernel takes it (by value). A Row is
// also what the fused path's second stage probes with: its intermediate
// row, held in registers.
struct DeltaView {
  const u64 *keys;
  const u8 *vals;  // null when the stream carries no val
  u32 vb;
  const u64 *times;
  const i64 *diffs;
  u64 n;
  u32 kw;
  struct Row {
    const u64 *key;
    const u8 *val;
    u64 t;
    i64 d;
  };
  __device__ __forceinline__ Row row(u64 i) const {
    return {keys + i * kw, vals ? vals + i * vb : nullptr, times[i],
            diffs[i]};
  }
};

// Time mode. A PM_JOIN probe and an allpass batch keep every update; the
// half-join modes keep those with t2 <= t (le) or t2 < t (lt).
// Number of kept updates in [lo, hi):
__device__ __forceinline__ u32 d_time_count(const DevBatch &b, int allpass,
                                            int mode, u32 lo, u32 hi,
                                            u64 t) {
  if (mode == PM_JOIN || allpass) return hi - lo;
  u32 m = 0;
  for (u32 u = lo; u < hi; u++) {
    u64 t2 = b.times[u];
    m += (mode == PM_HALF_LE) ? (t2 <= t) : (t2 < t);
  }
  return m;
}

// Output time of update u in *tout, or false when the mode filters it.
__device__ __forceinline__ bool d_time_out(const DevBatch &b, int allpass,
                                           int mode, u32 u, u64 t,
                                           u64 *tout) {
  *tout = t;
  if (allpass) return true;
  u64 t2 = b.times[u];
  if (mode == PM_JOIN) {
    if (t2 > t) *tout = t2;
    return true;
  }
  return (mode == PM_HALF_LE) ? (t2 <= t) : (t2 < t);
}

// Wave-aggregated output-queue reservation: exclusive prefix of c across
// the wavefront, one atomicAdd per wave. ALL 64 lanes must participate.
__device__ __forceinline__ u64 wave_reserve(unsigned long long *ctr, u32 c,
                                            u32 lane) {
  u32 pre = c;
  for (int d = 1; d < 64; d <<= 1) {
    u32 up = __shfl_up(pre, d, 64);
    if ((int)lane >= d) pre += up;
  }
  u32 excl = pre - c;
  unsigned long long wtotal = (unsigned long long)(u32)__shfl((int)pre, 63,
                                                              64);
  long long basell = 0;
  if (lane == 63 && wtotal)
    basell = (long long)atomicAdd(ctr, wtotal);
  return (u64)__shfl((int64_t)basell, 63, 64) + excl;
}

// Device half of the probe protocol: reserve c entries
// of the first queue and e of the second (ALL 64 lanes must call), and
// tell whether this lane has anything to write and both slices fit.
// ctr[0]/ctr[1] accumulate the EXACT totals whether or not a slice fits;
// a lane whose slice would cross a capacity skips its writes, and the
// host relaunches once at the exact counts.
__device__ __forceinline__ bool queue_reserve(unsigned long long *ctr,
                                              u64 cap, u64 cap2, u32 c,
                                              u32 e, u32 lane, u64 *o,
                                              u64 *eo) {
  *o = wave_reserve(ctr, c, lane);
  *eo = wave_reserve(ctr + 1, e, lane);
  return (c | e) && *o + c <= cap && *eo + e <= cap2;
}

// The fixed-width probes' output, passed to the kernels by value: an
// ok-row queue of cap rows and an error-row queue of ecap rows.
struct EmitQueue {
  u64 cap, ecap;
  unsigned long long *ctr;  // [0] ok rows, [1] error rows
  u64 *okeys;
  u8 *ovals;
  u64 *otimes;
  i64 *odiffs;
  u64 *ecodes, *etimes;
  i64 *ediffs;
  __device__ __forceinline__ bool reserve(u32 c, u32 e, u32 lane, u64 *o,
                                          u64 *eo) const {
    return queue_reserve(ctr, cap, ecap, c, e, lane, o, eo);
  }
};

// Count the output rows of one (delta row, batch) pair: walk the key's
// val range applying the closure filter and the time mode. Returns
// ok_count | err_count << 32 (err = closure evaluation errors, the
// could_error split of linear_join.rs:495-541).
__device__ __forceinline__ u64 d_count_pair(const DevBatch &b, int allpass,
                                            const DeltaView::Row &r,
                                            u64 kvr, int mode, int swap,
                                            const mz_gpu_closure &cl,
                                            u32 lvb) {
  u32 c = 0, e = 0;
  for (u32 j = (u32)kvr; j < (u32)(kvr >> 32); j++) {
    const u8 *lv = b.vals ? b.vals + (u64)j * lvb : nullptr;
    const u8 *v1 = swap ? lv : r.val;
    const u8 *v2 = swap ? r.val : lv;
    int cls = d_closure_apply(&cl, r.key, v1, v2, nullptr, nullptr);
    if (cls == 0) continue;
    u32 m = d_time_count(b, allpass, mode, b.vu_off[j], b.vu_off[j + 1], r.t);
    if (cls == 1)
      c += m;
    else
      e += m;
  }
  return (u64)c | ((u64)e << 32);
}

// Emit the counted rows at queue offsets *o (ok) / *eo (err) — ok fields
// written straight to global (closure filters run before any field
// write); error rows carry (code, time, d1*d2).
__device__ __forceinline__ void d_emit_pair(const DevBatch &b, int allpass,
                                            const DeltaView::Row &r,
                                            u64 kvr, int mode, int swap,
                                            const mz_gpu_closure &cl,
                                            u32 lvb, u32 okw, u32 ovb,
                                            const EmitQueue &q, u64 *o,
                                            u64 *eo) {
  for (u32 j = (u32)kvr; j < (u32)(kvr >> 32); j++) {
    const u8 *lv = b.vals ? b.vals + (u64)j * lvb : nullptr;
    const u8 *v1 = swap ? lv : r.val;
    const u8 *v2 = swap ? r.val : lv;
    int cls = d_closure_apply(&cl, r.key, v1, v2, nullptr, nullptr);
    if (cls == 0) continue;
    for (u32 u = b.vu_off[j]; u < b.vu_off[j + 1]; u++) {
      u64 tout;
      if (!d_time_out(b, allpass, mode, u, r.t, &tout)) continue;
      if (cls == 2) {
        q.ecodes[*eo] = MZ_ERR_DIVISION_BY_ZERO;
        q.etimes[*eo] = tout;
        q.ediffs[*eo] = wmul(r.d, b.diffs[u]);
        (*eo)++;
        continue;
      }
      (void)d_closure_apply(&cl, r.key, v1, v2, q.okeys + *o * okw,
                            q.ovals + *o * ovb);
      q.otimes[*o] = tout;
      q.odiffs[*o] = wmul(r.d, b.diffs[u]);
      (*o)++;
    }
  }
}

// canonical key order: i64-tuple ascending
__device__ __forceinline__ int d_key_cmp(const u64 *a, const u64 *b,
                                         u32 kw) {
  for (u32 w = 0; w < kw; w++) {
    i64 x = (i64)a[w], y = (i64)b[w];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

// Single-walk probe (DESIGN §9 candidate (b), the half_join2 probe loop
// replacement, delta_join.rs:500,544): one kernel probes AND emits —
// each (row, batch) pair counts its matches from the just-read range
// (L2-hot), reserves a slice of the output queue with one wave-
// aggregated atomic, and writes. Halves the probe pair's HBM traffic
// versus count+scan+emit: the delta tuple, hash line, val range and upd
// ranges are each touched once cold. Output order is queue order (non-
// deterministic); every consumer consolidates (canonical sort), so
// results are unchanged — parity holds on consolidated outputs.
// *ctr always accumulates the EXACT total match count; writes are
// skipped when a slice would cross `cap`, and the host relaunches with
// cap = exact count on overflow (rare; capacity hint kept per
// arrangement).
#define PROBE_TILE 4
__global__ void k_probe_walk(DeltaView d, u32 lvb, BatchList bl, int mode,
                             int swap, const mz_gpu_closure cl,
                             EmitQueue q) {
  u32 okw = cl.out.key_words, ovb = cl.out.val_bytes;
  u64 n = d.n;
  u64 total = n * (u64)bl.n;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (total + stride - 1) / stride;  // uniform across the wave
  u32 lane = threadIdx.x & 63;
  // PROBE_TILE pairs per macro-iteration: phase A issues up to 4
  // independent random hash-line reads per thread (MLP), phases B/C walk
  // the L2-hot ranges; ONE wave-aggregated reservation per tile keeps
  // lockstep convergence off the per-pair critical path.
  for (u64 it0 = 0; it0 < iters; it0 += PROBE_TILE) {
    u64 kvr[PROBE_TILE];
    u64 cc[PROBE_TILE];
    // Phase A: hash lookups (independent random lines in flight)
#pragma unroll
    for (int tt = 0; tt < PROBE_TILE; tt++) {
      u64 idx = start + (it0 + tt) * stride;
      kvr[tt] = ~0ull;
      cc[tt] = 0;
      if (it0 + tt < iters && idx < total) {
        int bi = (int)(idx / n);
        const DevBatch &b = bl.b[bi];
        kvr[tt] = hash_lookup_range(b.hash, b.hash_slots,
                                    d.keys + (idx % n) * d.kw, d.kw);
      }
    }
    // Phase B: count matches per slot (filters applied); low 32 bits ok
    // rows, high 32 error rows
    u32 csum = 0, esum = 0;
#pragma unroll
    for (int tt = 0; tt < PROBE_TILE; tt++) {
      if (kvr[tt] == ~0ull) continue;
      u64 idx = start + (it0 + tt) * stride;
      u64 i = idx % n;
      int bi = (int)(idx / n);
      cc[tt] = d_count_pair(bl.b[bi], bl.allpass[bi], d.row(i), kvr[tt],
                            mode, swap, cl, lvb);
      csum += (u32)cc[tt];
      esum += (u32)(cc[tt] >> 32);
    }
    u64 o, eo;
    if (!q.reserve(csum, esum, lane, &o, &eo)) continue;
    // Phase C: emit from L2-hot lines, fields written straight to the
    // reserved global slots (closure filters run before any field write)
#pragma unroll
    for (int tt = 0; tt < PROBE_TILE; tt++) {
      if (cc[tt] == 0) continue;
      u64 idx = start + (it0 + tt) * stride;
      u64 i = idx % n;
      int bi = (int)(idx / n);
      d_emit_pair(bl.b[bi], bl.allpass[bi], d.row(i), kvr[tt], mode, swap,
                  cl, lvb, okw, ovb, q, &o, &eo);
    }
  }
}

// Full-scan peek walk (IndexPeek without literal constraints,
// compute_state.rs): the batches are walked, not hashed into. One work
// item per (batch, val index j) over the whole BatchList; vbase.v[b] is the
// first item of batch b (vbase.v[bl.n] = the total), so an item finds its
// batch by a linear search of at most 12 entries. The item's updates at
// t' <= as_of are summed (wrapping) and ONE row per val leaves with time
// as_of and that sum — the host consolidates across batches. Consecutive
// lanes read consecutive val_key / vals / vu_off; keys and times/diffs are
// near-monotone gathers. Every lane of a wave runs the same number of
// iterations and reaches q.reserve in each (idle lanes with c = e = 0).
struct ScanBases {
  u64 v[13];
};

__global__ void k_scan_walk(BatchList bl, ScanBases vbase, u32 kw, u32 vb,
                            u64 as_of, const mz_gpu_closure cl,
                            EmitQueue q) {
  u32 okw = cl.out.key_words, ovb = cl.out.val_bytes;
  u64 total = vbase.v[bl.n];
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (total + stride - 1) / stride;  // uniform across the wave
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 idx = start + it * stride;
    const u64 *key = nullptr;
    const u8 *val = nullptr;
    i64 s = 0;
    int cls = 0;
    if (idx < total) {
      int bi = 0;
      while (bi + 1 < bl.n && idx >= vbase.v[bi + 1]) bi++;
      const DevBatch &b = bl.b[bi];
      u64 j = idx - vbase.v[bi];
      key = b.keys + (u64)b.val_key[j] * kw;
      val = vb ? b.vals + j * vb : nullptr;
      cls = d_closure_apply(&cl, key, nullptr, val, nullptr, nullptr);
      if (cls) {
        u32 lo = b.vu_off[j], hi = b.vu_off[j + 1];
        if (bl.allpass[bi]) {
          for (u32 u = lo; u < hi; u++) s = wadd(s, b.diffs[u]);
        } else {
          for (u32 u = lo; u < hi; u++)
            if (b.times[u] <= as_of) s = wadd(s, b.diffs[u]);
        }
      }
    }
    u32 c = (cls == 1 && s != 0) ? 1u : 0u;
    u32 e = (cls == 2 && s != 0) ? 1u : 0u;
    u64 o, eo;
    if (!q.reserve(c, e, lane, &o, &eo)) continue;
    if (c) {  // count mode checked every erroring compute: this returns 1
      (void)d_closure_apply(&cl, key, nullptr, val, q.okeys + o * okw,
                            q.ovals + o * ovb);
      q.otimes[o] = as_of;
      q.odiffs[o] = s;
    } else {
      q.ecodes[eo] = MZ_ERR_DIVISION_BY_ZERO;
      q.etimes[eo] = as_of;
      q.ediffs[eo] = s;
    }
  }
}

// Count the negative ones among n diffs into *flag (the peek's "saw
// retractions for a row that does not exist" check).
__global__ void k_any_negative(const i64 *diffs, u64 n,
                               unsigned long long *flag) {
  GRID_STRIDE(i, n) {
    if (diffs[i] < 0) atomicAdd(flag, 1ull);
  }
}

// ------------------------------------------------------ temporal filter
// MfpPlan::evaluate (src/expr/src/linear.rs) restated: the mz_now() bounds
// of a temporal MapFilterProject give each input update a validity
// interval [lo, hi) and turn it into up to two output updates, +d at lo and
// -d at hi. The bounds travel by value.
struct TemporalBounds {
  u32 n;
  mz_gpu_time_bound b[MZ_GPU_MAX_BOUNDS];
  u64 until;
};

// The operator's third queue next to an EmitQueue: the updates at or beyond
// the push's upper, which stay held. Its row counter is q.ctr[2]; q.ctr[3]
// counts input times outside [lower, upper).
struct HeldQueue {
  u64 cap;
  u64 *keys;
  u8 *vals;
  u64 *times;
  i64 *diffs;
};

// One row's window, bounds evaluated in spec order (mz_gpu.h, row semantics
// 2-3). Returns 0 = the row yields nothing (a NULL bound or an empty
// window), 1 = [*lo, *hi) with *has_hi telling whether an upper bound
// exists, 2 = a bound is not an mz_timestamp (the error row).
__device__ __forceinline__ int d_temporal_window(const TemporalBounds &tb,
                                                 const u64 *key,
                                                 const u8 *val, u64 t,
                                                 u64 *lo, u64 *hi,
                                                 bool *has_hi) {
  u64 l = t, h = 0;
  bool hh = false;
  for (u32 i = 0; i < tb.n; i++) {
    const mz_gpu_time_bound b = tb.b[i];
    const u8 *p = (b.src == MZ_SRC_KEY ? (const u8 *)key : val) + b.off;
    if (b.nullable && p[b.width] != 0) return 0;
    // datum + add in 128 bits: [-2^64, 2^64 - 2], never wrapped
    i128 v = (i128)d_read_int(p, b.width) + (i128)b.add;
    if (v < 0) return 2;
    u64 u = (u64)v;
    if (b.kind == MZ_TB_LOWER) {
      if (u > l) l = u;
    } else if (!hh || u < h) {
      h = u;
      hh = true;
    }
  }
  *lo = l;
  *hi = h;
  *has_hi = hh;
  return (hh && h <= l) ? 0 : 1;
}

// Slot `idx` of the ready queue (when the update's time is below the push's
// upper) or of the held queue: writes time and diff and hands back where
// the row's key and val go.
struct RowSlot {
  u64 *k;
  u8 *v;
};
__device__ __forceinline__ RowSlot d_temporal_slot(bool ready,
                                                   const EmitQueue &q,
                                                   const HeldQueue &h,
                                                   u32 okw, u32 ovb, u64 idx,
                                                   u64 time, i64 diff) {
  if (ready) {
    q.otimes[idx] = time;
    q.odiffs[idx] = diff;
    return {q.okeys + idx * okw, q.ovals + idx * ovb};
  }
  h.times[idx] = time;
  h.diffs[idx] = diff;
  return {h.keys + idx * okw, h.vals + idx * ovb};
}

// One work item per input update (grid-stride). A lane counts what its row
// emits — c_ready and c_held in {0,1,2} ok rows, e in {0,1} error rows —
// and the wave reserves its slices of the three queues; the fields go
// straight to the reserved slots. The queues are sized at their exact
// bounds (2n ready, 2n held beyond what the held queue already has, n
// errors), so nothing overflows and nothing is relaunched. Every lane of a
// wave runs the same number of iterations and reaches both reservations in
// each one (the row index is clamped; idle lanes reserve nothing).
// The closure's filters run in count mode first; its projection runs once
// per emitting row, into the row's first slot, and a two-update row's second
// slot is a copy of the first.
__global__ void k_temporal_eval(DeltaView d, u64 lower, u64 upper,
                                const mz_gpu_closure cl,
                                const TemporalBounds tb, EmitQueue q,
                                HeldQueue h) {
  u32 okw = cl.out.key_words, ovb = cl.out.val_bytes;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (d.n + stride - 1) / stride;  // uniform across the wave
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 idx = start + it * stride;
    bool valid = idx < d.n;
    const DeltaView::Row r = d.row(valid ? idx : d.n - 1);
    u64 lo = 0, hi = 0;
    bool e_lo = false, e_hi = false;  // the +d and the -d update
    u32 e = 0;
    if (valid) {
      if (r.t < lower || r.t >= upper) {
        atomicAdd(q.ctr + 3, 1ull);  // the host refuses the push
      } else if (d_closure_apply(&cl, r.key, r.val, nullptr, nullptr,
                                 nullptr)) {
        bool has_hi;
        int w = d_temporal_window(tb, r.key, r.val, r.t, &lo, &hi, &has_hi);
        if (w == 2) {
          e = 1;
        } else if (w == 1) {
          e_lo = lo < tb.until;
          e_hi = has_hi && hi < tb.until;
        }
      }
    }
    bool r_lo = e_lo && lo < upper, r_hi = e_hi && hi < upper;
    u32 c_ready = (u32)r_lo + (u32)r_hi;
    u32 c_held = (u32)(e_lo && !r_lo) + (u32)(e_hi && !r_hi);
    u64 o, eo;
    (void)q.reserve(c_ready, e, lane, &o, &eo);
    u64 ho = wave_reserve(q.ctr + 2, c_held, lane);
    // the capacities are exact bounds; a slice past one is never written
    if (!(c_ready | c_held | e) || o + c_ready > q.cap || eo + e > q.ecap ||
        ho + c_held > h.cap)
      continue;
    if (e) {  // emitted at the input time, never held
      q.ecodes[eo] = MZ_ERR_TIMESTAMP_OUT_OF_RANGE;
      q.etimes[eo] = r.t;
      q.ediffs[eo] = r.d;
      continue;
    }
    RowSlot s0{nullptr, nullptr}, s1{nullptr, nullptr};
    if (e_lo) {
      s0 = d_temporal_slot(r_lo, q, h, okw, ovb, r_lo ? o : ho, lo, r.d);
      (r_lo ? o : ho)++;
    }
    if (e_hi) {  // the negation wraps, as Diff does
      RowSlot s = d_temporal_slot(r_hi, q, h, okw, ovb, r_hi ? o : ho, hi,
                                  (i64)(0 - (u64)r.d));
      (e_lo ? s1 : s0) = s;
    }
    (void)d_closure_apply(&cl, r.key, r.val, nullptr, s0.k, s0.v);
    if (s1.k) {
      for (u32 w = 0; w < okw; w++) s1.k[w] = s0.k[w];
      for (u32 c = 0; c < ovb; c++) s1.v[c] = s0.v[c];
    }
  }
}

// One pass over the resident held columns (kw/vb = the operator's output
// schema): a row whose time is below `upper` is appended to the ready
// queue, every other row to the held queue — the same wave-aggregated
// reservations as k_temporal_eval, on the same counters.
__global__ void k_temporal_release(const u64 *keys, const u8 *vals,
                                   const u64 *times, const i64 *diffs, u64 n,
                                   u32 kw, u32 vb, u64 upper, EmitQueue q,
                                   HeldQueue h) {
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (n + stride - 1) / stride;  // uniform across the wave
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 idx = start + it * stride;
    bool valid = idx < n;
    u64 i = valid ? idx : n - 1;
    u64 t = times[i];
    bool rdy = valid && t < upper, stay = valid && !rdy;
    u64 o = wave_reserve(q.ctr, rdy ? 1u : 0u, lane);
    u64 ho = wave_reserve(q.ctr + 2, stay ? 1u : 0u, lane);
    if (!valid || (rdy ? o >= q.cap : ho >= h.cap)) continue;
    RowSlot s = d_temporal_slot(rdy, q, h, kw, vb, rdy ? o : ho, t, diffs[i]);
    for (u32 w = 0; w < kw; w++) s.k[w] = keys[i * kw + w];
    for (u32 c = 0; c < vb; c++) s.v[c] = vals[i * vb + c];
  }
}

// ------------------------------------------- scalar-expression MFP (device)
// The postfix interpreter of mz_gpu_mfp_spec (mz_gpu.h states the
// semantics). A value is (i64, tag): tag 0 datum, 1 NULL, 1 + MZ_ERR_* an
// error. Everything is evaluated eagerly and the lazy operators select, so
// the program counter, the stack pointer and the opcode switch are uniform
// across the wave; only data differs between lanes.
struct XVal {
  i64 v;
  u32 t;
};
#define XERR(code) (1u + (u32)(code))

__device__ __forceinline__ XVal d_x_unary(u8 op, XVal a) {
  if (a.t >= 2) return {0, a.t};
  if (op == MZ_X_IS_NULL) return {(i64)(a.t == 1), 0};
  if (a.t) return {0, 1};
  if (op == MZ_X_NOT) return {(i64)(a.v == 0), 0};
  if (a.v == INT64_MIN) return {0, XERR(MZ_ERR_INT64_OUT_OF_RANGE)};
  return {(op == MZ_X_ABS && a.v >= 0) ? a.v : -a.v, 0};
}

__device__ __forceinline__ XVal d_x_binary(u8 op, XVal a, XVal b) {
  if (op == MZ_X_COALESCE) return a.t == 1 ? b : a;
  if (op == MZ_X_AND || op == MZ_X_OR) {
    i64 dom = op == MZ_X_OR;  // the operand value that decides alone
    if ((a.t == 0 && a.v == dom) || (b.t == 0 && b.v == dom)) return {dom, 0};
    if (a.t >= 2) return {0, a.t};
    if (b.t >= 2) return {0, b.t};
    if (a.t | b.t) return {0, 1};
    return {1 - dom, 0};
  }
  if (a.t >= 2) return {0, a.t};
  if (b.t >= 2) return {0, b.t};
  if (a.t | b.t) return {0, 1};
  i64 x = a.v, y = b.v, r = 0;
  switch (op) {
    case MZ_X_ADD:
      if (__builtin_add_overflow(x, y, &r))
        return {0, XERR(MZ_ERR_NUMERIC_FIELD_OVERFLOW)};
      break;
    case MZ_X_SUB:
      if (__builtin_sub_overflow(x, y, &r))
        return {0, XERR(MZ_ERR_NUMERIC_FIELD_OVERFLOW)};
      break;
    case MZ_X_MUL:
      if (__builtin_mul_overflow(x, y, &r))
        return {0, XERR(MZ_ERR_NUMERIC_FIELD_OVERFLOW)};
      break;
    case MZ_X_DIV:
    case MZ_X_MOD: {
      if (y == 0) return {0, XERR(MZ_ERR_DIVISION_BY_ZERO)};
      if (y == -1) {  // the one quotient that does not fit
        if (op == MZ_X_MOD) return {0, 0};
        if (x == INT64_MIN) return {0, XERR(MZ_ERR_INT64_OUT_OF_RANGE)};
        return {-x, 0};
      }
      i64 q = x / y;  // truncates toward zero; y is neither 0 nor -1
      r = op == MZ_X_DIV ? q : x - q * y;
      break;
    }
    case MZ_X_LT: r = x < y; break;
    case MZ_X_LE: r = x <= y; break;
    case MZ_X_GT: r = x > y; break;
    case MZ_X_GE: r = x >= y; break;
    case MZ_X_EQ: r = x == y; break;
    default: r = x != y; break;  // MZ_X_NE
  }
  return {r, 0};
}

// Run the program over one input row. The lane's stack is its column of
// the block's LDS arrays: slot s lives at lv[s * BLK] / lt[s * BLK] (lv and
// lt already offset by threadIdx.x), so a lane touches no other lane's
// entries, consecutive lanes hit consecutive banks and no barrier is
// needed. Returns the row's class: 0 dropped, 1 ok, 1 + MZ_ERR_* an error
// row. STORE = false classifies only; STORE = true also writes the OUT
// fields to okey / oval, and is run on rows classified ok.
template <bool STORE>
__device__ __forceinline__ u32 d_mfp_run(const mz_gpu_mfp_spec &P,
                                         const u64 *key, const u8 *val,
                                         u64 *okey, u8 *oval, i64 *lv,
                                         u8 *lt) {
  u32 cls = 1;
  u32 sp = 0;  // uniform: create-time validation simulated it
  auto pop = [&]() -> XVal {
    sp--;
    return {lv[sp * BLK], (u32)lt[sp * BLK]};
  };
  auto push = [&](XVal x) {
    lv[sp * BLK] = x.v;
    lt[sp * BLK] = (u8)x.t;
    sp++;
  };
  for (u32 pc = 0; pc < P.n_ops; pc++) {
    const mz_gpu_xop op = P.ops[pc];  // wave-uniform: scalar loads
    switch (op.op) {
      case MZ_X_COL: {
        const u8 *p = (op.src == MZ_SRC_KEY ? (const u8 *)key : val) + op.off;
        XVal x{0, 0};
        if (op.nullable && p[op.width] != 0)
          x.t = 1;
        else if (op.width == 1)
          x.v = p[0] != 0;
        else
          x.v = d_read_int(p, op.width);
        push(x);
        break;
      }
      case MZ_X_LIT: push({op.imm, 0}); break;
      case MZ_X_NULL: push({0, 1}); break;
      case MZ_X_NEG:
      case MZ_X_ABS:
      case MZ_X_NOT:
      case MZ_X_IS_NULL: push(d_x_unary(op.op, pop())); break;
      case MZ_X_IF: {
        XVal e = pop(), t = pop(), c = pop();
        push(c.t >= 2 ? XVal{0, c.t} : (c.t == 0 && c.v != 0) ? t : e);
        break;
      }
      case MZ_X_FILTER: {
        XVal x = pop();
        if (cls == 1) {
          if (x.t >= 2)
            cls = x.t;
          else if (x.t == 1 || x.v == 0)
            cls = 0;
        }
        break;
      }
      case MZ_X_OUT: {
        XVal x = pop();
        if (!STORE) {
          if (cls != 1) break;
          if (x.t >= 2)
            cls = x.t;
          else if (x.t == 1 && !op.nullable)
            cls = XERR(MZ_ERR_UNEXPECTED_NULL);
          else if (x.t == 0 && op.width == 4 && x.v != (i64)(int32_t)x.v)
            cls = XERR(MZ_ERR_INT32_OUT_OF_RANGE);
          break;
        }
        u8 *dst = (op.src == 0 ? (u8 *)okey : oval) + op.off;
        i64 v = x.t ? 0 : x.v;  // NULL: zero datum bytes
        if (op.width == 8) {
          memcpy(dst, &v, 8);
        } else if (op.width == 4) {
          int32_t w = (int32_t)v;
          memcpy(dst, &w, 4);
        } else {
          dst[0] = (u8)v;
        }
        if (op.nullable) dst[op.width] = (u8)(x.t == 1);
        break;
      }
      default: {  // the binary operators
        XVal b = pop(), a = pop();
        push(d_x_binary(op.op, a, b));
        break;
      }
    }
  }
  return cls;
}

// Grid-stride over the input updates, as k_temporal_eval: every lane of a
// wave runs the same number of iterations and reaches the one reservation
// in each (row indices are clamped; idle lanes reserve nothing). A lane
// takes MFP_ROWS rows per iteration, a grid stride apart, so that loads stay
// coalesced: a classify pass without stores gives each row's class, the
// wave reserves once for all of them — the counters are one address each
// and returning atomics on one address serialise, so reservations, not
// bytes, are what this kernel pays for — and then the ok rows
// run the program again with OUT storing straight to the reserved slots and
// the error rows write (code, time, diff). An input row yields at most one
// row, in exactly one queue, so both queues are sized at the exact bound n:
// nothing overflows and nothing is relaunched.
#define MFP_ROWS 8
__global__ void __launch_bounds__(BLK)
    k_mfp_eval(DeltaView d, const mz_gpu_mfp_spec P, EmitQueue q) {
  __shared__ i64 s_lv[MZ_GPU_XSTACK * BLK];
  __shared__ u8 s_lt[MZ_GPU_XSTACK * BLK];
  i64 *lv = s_lv + threadIdx.x;
  u8 *lt = s_lt + threadIdx.x;
  u32 okw = P.out.key_words, ovb = P.out.val_bytes;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 span = stride * MFP_ROWS;
  u64 iters = (d.n + span - 1) / span;  // uniform across the wave
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 base = start + it * span;
    u32 classes = 0;  // 4 bits per row: 0 dropped, 1 ok, 1 + MZ_ERR_*
    u32 c = 0, e = 0;
#pragma unroll 1
    for (u32 j = 0; j < MFP_ROWS; j++) {
      u64 idx = base + j * stride;
      if (idx - lane >= d.n) break;  // the whole wave is past the end
      bool valid = idx < d.n;
      const DeltaView::Row r = d.row(valid ? idx : d.n - 1);
      u32 cls = d_mfp_run<false>(P, r.key, r.val, nullptr, nullptr, lv, lt);
      if (!valid) cls = 0;
      classes |= cls << (4 * j);
      c += cls == 1;
      e += cls >= 2;
    }
    u64 o, eo;
    (void)q.reserve(c, e, lane, &o, &eo);
    // the capacities are exact bounds; a slot past one is never written
    if (o + c > q.cap || eo + e > q.ecap) continue;
#pragma unroll 1
    for (u32 j = 0; j < MFP_ROWS && (classes >> (4 * j)); j++) {
      u32 cls = (classes >> (4 * j)) & 15;
      if (cls == 0) continue;
      const DeltaView::Row r = d.row(base + j * stride);
      if (cls == 1) {
        (void)d_mfp_run<true>(P, r.key, r.val, q.okeys + o * okw,
                              q.ovals + o * ovb, lv, lt);
        q.otimes[o] = r.t;
        q.odiffs[o] = r.d;
        o++;
      } else {
        q.ecodes[eo] = cls - 1;
        q.etimes[eo] = r.t;
        q.ediffs[eo] = r.d;
        eo++;
      }
    }
  }
}

// Smallest of the first *np times into *out (which starts at ~0): the
// held buffer's next release time, read back with the push's closing copy.
__global__ void k_time_min(const u64 *times, const u64 *np,
                           unsigned long long *out) {
  u64 n = *np, m = ~0ull;
  GRID_STRIDE(i, n) m = times[i] < m ? times[i] : m;
  for (int s = 32; s; s >>= 1) {
    u64 other = (u64)__shfl_xor((int64_t)m, s, 64);
    m = other < m ? other : m;
  }
  if ((threadIdx.x & 63) == 0 && m != ~0ull) atomicMin(out, m);
}

// Fused two-stage delta-path probe (one delta path's two lookup stages,
// delta_join.rs:338-472, in a single kernel): a stage-1 match produces
// its intermediate (key2, val2) in REGISTERS and immediately probes the
// stage-2 arrangement — the intermediate stream is never materialized in
// HBM, and the per-stage launch + counter-readback round trip
// disappears. Half-join modes only (le/lt per stage, no swap): times are
// total-ordered u64s and each stage's time filter keeps t2 (<=|<) t, so
// the promoted output time stays the delta time t and the stage-2 filter
// compares against the same t (delta_join.rs:157-160,362,372). Counting
// and emission walk the same nested ranges (emission L2-hot); *ctr[0/1]
// always accumulate exact ok/err totals (host relaunches on overflow),
// ctr[2] counts intermediate rows (stats/roofline only).
#define P2_MAX_KW 2
#define P2_MAX_VB 48

// Count one (delta row, stage-1 batch) pair's final emissions through
// both stages; returns ok | err<<32 and adds this pair's intermediate
// row count to *inter (stats).
__device__ __forceinline__ u64 d_path2_count(
    const DeltaView::Row &r, const DevBatch &b1, int allpass1, u64 kvr1,
    int mode1, const mz_gpu_closure &cl1, u32 lvb1, u32 k2w,
    const BatchList &bl2, int mode2, const mz_gpu_closure &cl2, u32 lvb2,
    u64 *inter) {
  u32 c = 0, e = 0;
  for (u32 j = (u32)kvr1; j < (u32)(kvr1 >> 32); j++) {
    const u8 *lv = b1.vals ? b1.vals + (u64)j * lvb1 : nullptr;
    int cls = d_closure_apply(&cl1, r.key, r.val, lv, nullptr, nullptr);
    if (cls == 0) continue;
    u32 m1 = d_time_count(b1, allpass1, mode1, b1.vu_off[j],
                          b1.vu_off[j + 1], r.t);
    if (m1 == 0) continue;
    if (cls == 2) {
      e += m1;
      continue;
    }
    *inter += m1;
    u64 k2[P2_MAX_KW];
    u8 v2buf[P2_MAX_VB];
    (void)d_closure_apply(&cl1, r.key, r.val, lv, k2, v2buf);
    for (int b2i = 0; b2i < bl2.n; b2i++) {
      const DevBatch &b2 = bl2.b[b2i];
      u64 kvr2 = hash_lookup_range(b2.hash, b2.hash_slots, k2, k2w);
      if (kvr2 == ~0ull) continue;
      u64 ce2 = d_count_pair(b2, bl2.allpass[b2i], {k2, v2buf, r.t, 0}, kvr2,
                             mode2, 0, cl2, lvb2);
      c += m1 * (u32)ce2;
      e += m1 * (u32)(ce2 >> 32);
    }
  }
  return (u64)c | ((u64)e << 32);
}

// Emit one pair's rows at queue offsets *o / *eo (same nested walk as
// the count — ranges are L2-hot on this second pass).
__device__ __forceinline__ void d_path2_emit(
    const DeltaView::Row &r, const DevBatch &b1, int allpass1, u64 kvr1,
    int mode1, const mz_gpu_closure &cl1, u32 lvb1, u32 k2w,
    const BatchList &bl2, int mode2, const mz_gpu_closure &cl2, u32 lvb2,
    u32 okw, u32 ovb, const EmitQueue &q, u64 *o, u64 *eo) {
  for (u32 j = (u32)kvr1; j < (u32)(kvr1 >> 32); j++) {
    const u8 *lv = b1.vals ? b1.vals + (u64)j * lvb1 : nullptr;
    int cls = d_closure_apply(&cl1, r.key, r.val, lv, nullptr, nullptr);
    if (cls == 0) continue;
    u64 k2[P2_MAX_KW];
    u8 v2buf[P2_MAX_VB];
    if (cls == 1) (void)d_closure_apply(&cl1, r.key, r.val, lv, k2, v2buf);
    u32 lo = b1.vu_off[j], hi = b1.vu_off[j + 1];
    for (u32 u = lo; u < hi; u++) {
      // half-join modes never promote the time: a kept update's output
      // time is r.t itself
      u64 tout;
      if (!d_time_out(b1, allpass1, mode1, u, r.t, &tout)) continue;
      i64 d1 = wmul(r.d, b1.diffs[u]);
      if (cls == 2) {
        q.ecodes[*eo] = MZ_ERR_DIVISION_BY_ZERO;
        q.etimes[*eo] = r.t;
        q.ediffs[*eo] = d1;
        (*eo)++;
        continue;
      }
      for (int b2i = 0; b2i < bl2.n; b2i++) {
        const DevBatch &b2 = bl2.b[b2i];
        u64 kvr2 = hash_lookup_range(b2.hash, b2.hash_slots, k2, k2w);
        if (kvr2 == ~0ull) continue;
        d_emit_pair(b2, bl2.allpass[b2i], {k2, v2buf, r.t, d1}, kvr2, mode2,
                    0, cl2, lvb2, okw, ovb, q, o, eo);
      }
    }
  }
}

__global__ void k_probe_path2(DeltaView d, u32 lvb1, BatchList bl1,
                              int mode1, const mz_gpu_closure cl1, u32 lvb2,
                              BatchList bl2, int mode2,
                              const mz_gpu_closure cl2, EmitQueue q) {
  u32 okw = cl2.out.key_words, ovb = cl2.out.val_bytes;
  u32 k2w = cl1.out.key_words;
  u64 n = d.n;
  u64 total = n * (u64)bl1.n;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (total + stride - 1) / stride;  // uniform across the wave
  u32 lane = threadIdx.x & 63;
  // PROBE_TILE pairs per macro-iteration — the loop of k_probe_walk,
  // repeated here because sharing it through an inlined function cost
  // both kernels registers ("Probe-protocol refactor"):
  // phase A issues the independent stage-1 hash lines, phase B walks the
  // nested counts, ONE wave-aggregated reservation per tile, phase C
  // emits from L2-hot ranges.
  for (u64 it0 = 0; it0 < iters; it0 += PROBE_TILE) {
    u64 kvr1[PROBE_TILE];
    u64 cc[PROBE_TILE];
#pragma unroll
    for (int tt = 0; tt < PROBE_TILE; tt++) {
      u64 idx = start + (it0 + tt) * stride;
      kvr1[tt] = ~0ull;
      cc[tt] = 0;
      if (it0 + tt < iters && idx < total) {
        int bi = (int)(idx / n);
        const DevBatch &b = bl1.b[bi];
        kvr1[tt] = hash_lookup_range(b.hash, b.hash_slots,
                                     d.keys + (idx % n) * d.kw, d.kw);
      }
    }
    u32 csum = 0, esum = 0;
    u64 inter = 0;
#pragma unroll
    for (int tt = 0; tt < PROBE_TILE; tt++) {
      if (kvr1[tt] == ~0ull) continue;
      u64 idx = start + (it0 + tt) * stride;
      u64 i = idx % n;
      int bi = (int)(idx / n);
      cc[tt] = d_path2_count(d.row(i), bl1.b[bi], bl1.allpass[bi], kvr1[tt],
                             mode1, cl1, lvb1, k2w, bl2, mode2, cl2, lvb2,
                             &inter);
      csum += (u32)cc[tt];
      esum += (u32)(cc[tt] >> 32);
    }
    u64 o, eo;
    bool fits = q.reserve(csum, esum, lane, &o, &eo);
    if (inter) atomicAdd(q.ctr + 2, (unsigned long long)inter);
    if (!fits) continue;
#pragma unroll
    for (int tt = 0; tt < PROBE_TILE; tt++) {
      if (cc[tt] == 0) continue;
      u64 idx = start + (it0 + tt) * stride;
      u64 i = idx % n;
      int bi = (int)(idx / n);
      d_path2_emit(d.row(i), bl1.b[bi], bl1.allpass[bi], kvr1[tt], mode1,
                   cl1, lvb1, k2w, bl2, mode2, cl2, lvb2, okw, ovb, q, &o,
                   &eo);
    }
  }
}

// Merge probe for SORTED delta streams against one large batch: both
// sides are ascending in the canonical key order, so each block narrows
// the batch's key array to its delta rows' range with two binary
// searches, stages that window in LDS, and every thread resolves its
// rows' val ranges by an LDS search — the batch's keys/kv_off/vals/upds
// are then read in ASCENDING order across the grid (streaming) and the
// hash table is never touched. This is the sort-merge restatement of
// half_join2's per-key cursor seek (delta_join.rs:500,544;
// mz_join_core.rs:647-662) for the MI355X memory system: the measured
// uniform-random 128 B line ceiling is ~1.1 TB/s while sequential
// windows stream at HBM rates.
#define MERGE_DROWS 1024
#define MERGE_LDSW 8192
// Per-block key-window bounds for k_probe_merge, one THREAD per block
// (the in-block thread-0 search serialized ~21 dependent global loads
// while 255 lanes idled — measured 243 us/launch; precomputing all
// windows in one parallel kernel removes that).
__global__ void k_merge_bounds(const u64 *dkeys, u64 n, u32 kw,
                               const u64 *bkeys, u64 n_keys, u64 nblocks,
                               u64 *bounds) {
  GRID_STRIDE(blk, nblocks) {
    u64 r0 = blk * MERGE_DROWS;
    u64 r1 = r0 + MERGE_DROWS < n ? r0 + MERGE_DROWS : n;
    const u64 *k0 = dkeys + r0 * kw;
    const u64 *k1 = dkeys + (r1 - 1) * kw;
    u64 lo = 0, hi = n_keys;
    while (lo < hi) {
      u64 mid = (lo + hi) / 2;
      if (d_key_cmp(bkeys + mid * kw, k0, kw) < 0)
        lo = mid + 1;
      else
        hi = mid;
    }
    bounds[2 * blk] = lo;
    u64 lo2 = lo;
    hi = n_keys;
    while (lo2 < hi) {
      u64 mid = (lo2 + hi) / 2;
      if (d_key_cmp(bkeys + mid * kw, k1, kw) <= 0)
        lo2 = mid + 1;
      else
        hi = mid;
    }
    bounds[2 * blk + 1] = lo2;
  }
}

__global__ void k_probe_merge(DeltaView d, u32 lvb, DevBatch b, int allpass,
                              int mode, int swap, const mz_gpu_closure cl,
                              const u64 *bounds, EmitQueue q) {
  __shared__ u64 lk[MERGE_LDSW];
  u64 n = d.n;
  u32 kw = d.kw;
  u32 okw = cl.out.key_words, ovb = cl.out.val_bytes;
  u64 r0 = (u64)blockIdx.x * MERGE_DROWS;
  if (r0 >= n) return;
  u64 r1 = r0 + MERGE_DROWS < n ? r0 + MERGE_DROWS : n;
  u64 klo = bounds[2 * blockIdx.x], khi = bounds[2 * blockIdx.x + 1];
  u64 nk = khi - klo;
  bool use_lds = nk * kw <= MERGE_LDSW;
  if (use_lds) {
    for (u64 w = threadIdx.x; w < nk * kw; w += blockDim.x)
      lk[w] = b.keys[klo * kw + w];
    __syncthreads();
  }
  u32 lane = threadIdx.x & 63;
  const int RPT = MERGE_DROWS / BLK;  // rows per thread
  u64 kvr[RPT];
  u64 cc[RPT];
  u32 csum = 0, esum = 0;
  for (int s = 0; s < RPT; s++) {
    u64 i = r0 + threadIdx.x + (u64)s * blockDim.x;  // coalesced
    kvr[s] = ~0ull;
    cc[s] = 0;
    if (i < r1) {
      const u64 *key = d.keys + i * kw;
      const u64 *base = use_lds ? lk : b.keys + klo * kw;
      u64 lo = 0, hi = nk;
      while (lo < hi) {
        u64 mid = (lo + hi) / 2;
        if (d_key_cmp(base + mid * kw, key, kw) < 0)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo < nk && d_key_cmp(base + lo * kw, key, kw) == 0) {
        u64 kidx = klo + lo;
        kvr[s] = (u64)b.kv_off[kidx] | ((u64)b.kv_off[kidx + 1] << 32);
        cc[s] = d_count_pair(b, allpass, d.row(i), kvr[s], mode, swap, cl,
                             lvb);
        csum += (u32)cc[s];
        esum += (u32)(cc[s] >> 32);
      }
    }
  }
  u64 o, eo;
  if (!q.reserve(csum, esum, lane, &o, &eo)) return;
  for (int s = 0; s < RPT; s++) {
    if (!cc[s]) continue;
    u64 i = r0 + threadIdx.x + (u64)s * blockDim.x;
    d_emit_pair(b, allpass, d.row(i), kvr[s], mode, swap, cl, lvb, okw, ovb,
                q, &o, &eo);
  }
}

// Strict-weak ordering over expanded rows by global row id:
// (key i64-tuple, val LE-u64-tuple, time) — the engine's canonical order.
struct RowLess {
  const u64 *keys;
  const u8 *vals;
  const u64 *times;
  u32 kw, vb;
  __device__ bool operator()(u64 a, u64 b) const {
    for (u32 w = 0; w < kw; w++) {
      i64 x = (i64)keys[a * kw + w], y = (i64)keys[b * kw + w];
      if (x != y) return x < y;
    }
    for (u32 off = 0; off < vb; off += 8) {
      u64 x = le_val_word(vals + a * vb + off, vb - off);
      u64 y = le_val_word(vals + b * vb + off, vb - off);
      if (x != y) return x < y;
    }
    return times[a] < times[b];
  }
};

// expansion: flatten a DevBatch back to per-update (key,val,time,diff)
__global__ void k_expand_batch(DevBatch b, u32 kw, u32 vb, u64 frontier,
                               u64 *okeys, u8 *ovals, u64 *otimes,
                               i64 *odiffs, u64 base) {
  GRID_STRIDE(i, b.n_upds) {
    u32 v = b.upd_val[i];
    u32 k = b.val_key[v];
    u64 o = base + i;
    for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = b.keys[(u64)k * kw + w];
    for (u32 c = 0; c < vb; c++) ovals[o * vb + c] = b.vals[(u64)v * vb + c];
    u64 t = b.times[i];
    otimes[o] = t < frontier ? frontier : t;
    odiffs[o] = b.diffs[i];
  }
}

// ------------------------------------------------------------ partition

__global__ void k_shard_of(const u64 *keys, u32 kw, u64 n, u32 nshards,
                           u32 *shard) {
  GRID_STRIDE(i, n) shard[i] = (u32)(route_hash(keys + i * kw, kw) % nshards);
}

// ------------------------------------------------------------ reduce

// Accumulator per aggregate (Accum restatement, reduce.rs:1611-2270):
// 48 bytes: { u128 accum; u64 non_nulls, pos_infs, neg_infs, nans }.
struct Acc5 {
  u128 accum;
  u64 nn, pi, ni, nan;
};

__device__ __forceinline__ i128 d_float_to_fixed_point(double dv) {
  // reduce.rs:1663-1697 (wrapping trunc(n * 2^24) mod 2^128)
  u64 bits = __double_as_longlong(dv);
  u64 mantissa = bits & ((1ULL << 52) - 1);
  int exp_bits = (int)((bits >> 52) & 0x7ff);
  int exponent;
  if (exp_bits == 0) {
    exponent = -1074;
  } else {
    mantissa |= 1ULL << 52;
    exponent = exp_bits - 1075;
  }
  long e = (long)exponent + 24;
  u128 significand = (u128)mantissa;
  u128 magnitude;
  if (e >= 0)
    magnitude = e < 128 ? (significand << e) : (u128)0;
  else
    magnitude = (-e) < 128 ? (significand >> (-e)) : (u128)0;
  i128 m = (i128)magnitude;
  return (bits >> 63) ? (i128)(~(u128)m + 1) : m;
}

// exact round-to-nearest-even i128 -> double (matches host sitofp / Rust
// `as f64`, used by finalize SUM_F64, reduce.rs:1952)
__host__ __device__ inline double i128_to_double(i128 v) {
  if (v == 0) return 0.0;
  bool neg = v < 0;
  u128 m = neg ? (u128)0 - (u128)v : (u128)v;
  u64 hi = (u64)(m >> 64), lo = (u64)m;
  int bits;
#ifdef __HIP_DEVICE_COMPILE__
  bits = hi ? 128 - __clzll(hi) : 64 - __clzll(lo);
#else
  bits = hi ? 128 - __builtin_clzll(hi) : 64 - __builtin_clzll(lo);
#endif
  double d;
  if (bits <= 53) {
    d = (double)lo;
  } else {
    int shift = bits - 54;
    u64 top = (u64)(m >> shift);  // 54 bits
    bool sticky = (m & (((u128)1 << shift) - 1)) != 0;
    u64 mant = top >> 1;
    bool rnd = top & 1;
    if (rnd && (sticky || (mant & 1))) mant++;
    d = ldexp((double)mant, shift + 1);
  }
  return neg ? -d : d;
}

// datum -> Acc5 (datum_to_accumulator, reduce.rs:1699-1838)
__device__ __forceinline__ Acc5 d_datum_to_acc(const mz_gpu_aggregate a,
                                               const u8 *val) {
  Acc5 r{0, 0, 0, 0, 0};
  bool null = a.nullable && val[a.off + a.width] != 0;
  if (a.func == MZ_AGG_COUNT) {
    r.nn = null ? 0 : 1;
  } else if (a.func == MZ_AGG_SUM_I64) {
    if (!null) {
      r.accum = (u128)(i128)d_read_int(val + a.off, a.width);
      r.nn = 1;
    }
  } else {  // SUM_F64
    if (!null) {
      double n;
      if (a.width == 4) {
        float f;
        memcpy(&f, val + a.off, 4);
        n = (double)f;
      } else {
        memcpy(&n, val + a.off, 8);
      }
      r.nan = isnan(n) ? 1 : 0;
      r.pi = (n == HUGE_VAL) ? 1 : 0;
      r.ni = (n == -HUGE_VAL) ? 1 : 0;
      r.nn = 1;
      if (!r.nan && !r.pi && !r.ni) r.accum = (u128)d_float_to_fixed_point(n);
    }
  }
  return r;
}

// finalize one aggregate into its 24-byte output slot
// (finalize_accum, reduce.rs:1840-1997; slot layout DESIGN.md §2.1)
__device__ __forceinline__ void d_finalize(const mz_gpu_aggregate a,
                                           const Acc5 acc, i64 total,
                                           u8 *slot) {
  for (int i = 0; i < 24; i++) slot[i] = 0;
  bool zero = acc.accum == 0 && acc.nn == 0 && acc.pi == 0 && acc.ni == 0 &&
              acc.nan == 0;
  if (total > 0 && zero && a.func != MZ_AGG_COUNT) {
    slot[0] = 1;
    return;
  }
  if (a.func == MZ_AGG_COUNT) {
    i64 c = (i64)acc.nn;
    memcpy(slot + 8, &c, 8);
  } else if (a.func == MZ_AGG_SUM_I64) {
    u128 v = acc.accum;
    memcpy(slot + 8, &v, 16);
  } else {
    double v;
    // counts are SIGNED (Diff::is_positive, reduce.rs:1920-1927): a
    // wrapped-negative inf/nan count is NOT positive
    if ((i64)acc.nan > 0 || ((i64)acc.pi > 0 && (i64)acc.ni > 0))
      v = __longlong_as_double(0x7FF8000000000000LL);  // NaN
    else if ((i64)acc.pi > 0)
      v = HUGE_VAL;
    else if ((i64)acc.ni > 0)
      v = -HUGE_VAL;
    else
      v = i128_to_double((i128)acc.accum) / 16777216.0;
    memcpy(slot + 8, &v, 8);
  }
}

// Reduce state: open-addressing hash over persistent AccumRows.
//   slot words: [key kw][idx]
//   state row (u64 words): [key kw][total][na * 6 words of Acc5]
//
// Inserts are coherence-safe by construction: within one push, distinct
// keys are grouped so no two threads ever insert the same key; lookups and
// inserts run in SEPARATE kernel launches (kernel-boundary coherence —
// per-XCD L2s are not coherent within a launch, MI355X_MICROARCH §XCD),
// and the insert kernel's losers only CAS the idx word, never read another
// insert's key words. State row index = base + miss order (deterministic).
struct RedState {
  u64 *hash;
  u64 slots;
  u64 *rows;     // stride words
  u64 capacity;
  u32 stride_w;  // kw + 1 + 6*na
};

// Phase A: lookup each key group in the (fully published) table.
// G may be host-known (gidn == nullptr) or device-derived from gidn[m-1].
__global__ void k_red_lookup(const u64 *keys, u32 kw, const u32 *gstart,
                             u64 G, const u32 *gidn, u64 m, RedState st,
                             u32 *found, u32 *miss) {
  if (gidn) G = m ? gidn[m - 1] : 0;
  GRID_STRIDE(g, G) {
    const u64 *key = keys + (u64)gstart[g] * kw;
    int idx = hash_lookup(st.hash, st.slots, key, kw, kw + 1);
    found[g] = idx < 0 ? ~0u : (u32)idx;
    miss[g] = idx < 0 ? 1u : 0u;
  }
}

// Phase B: insert missing keys; row idx = base + rank among misses.
// base comes from *d_nrows when provided (bumped AFTER this launch);
// overflow sets *d_err instead of writing out of bounds.
__global__ void k_red_insert(const u64 *keys, u32 kw, const u32 *gstart,
                             u64 G, const u32 *gidn, u64 m,
                             const u32 *miss, const u32 *misspos, u64 base,
                             const u64 *d_nrows, u64 *d_err, RedState st) {
  if (gidn) G = m ? gidn[m - 1] : 0;
  if (d_nrows) base = *d_nrows;
  GRID_STRIDE(g, G) {
    if (!miss[g]) continue;
    const u64 *key = keys + (u64)gstart[g] * kw;
    u64 idx = base + misspos[g];
    if (idx >= st.capacity) {
      if (d_err) *d_err = 1;
      continue;
    }
    u64 *row = st.rows + idx * st.stride_w;
    for (u32 w = 0; w < kw; w++) row[w] = key[w];
    for (u32 w = kw; w < st.stride_w; w++) row[w] = 0;
    u64 h = route_hash(key, kw) & (st.slots - 1);
    for (;;) {
      u64 *slot = st.hash + h * (kw + 1);
      unsigned long long prev = atomicCAS((unsigned long long *)(slot + kw),
                                          ~0ull, (unsigned long long)idx);
      if (prev == ~0ull) {
        for (u32 w = 0; w < kw; w++) slot[w] = key[w];
        break;
      }
      h = (h + 1) & (st.slots - 1);
    }
  }
}

// ---- pieces shared by the two reduce apply kernels

// acc += c * d, all five components (explode_one * diff + semigroup
// merge; wrapping)
__device__ __forceinline__ void acc_fold(Acc5 &acc, const Acc5 c, i64 d) {
  acc.accum += c.accum * (u128)(i128)d;
  acc.nn += (u64)c.nn * (u64)d;
  acc.pi += (u64)c.pi * (u64)d;
  acc.ni += (u64)c.ni * (u64)d;
  acc.nan += (u64)c.nan * (u64)d;
}

// any component non-zero (reduce_abelian: keys with nonempty input
// accumulation produce one output row)
__device__ __forceinline__ bool acc_nonzero(const Acc5 &a) {
  return a.accum != 0 || a.nn || a.pi || a.ni || a.nan;
}

// A key whose old and new rows both exist and finalize to the same bytes
// emits nothing. When they differ: whether the new row comes before the old
// one in the canonical val order (le_val_word words, word 0 most
// significant, unsigned, zero-padded tail). Read off the same byte sweep:
// the first word that differs decides, and in it the highest byte.
__device__ __forceinline__ bool cancel_unchanged(bool &oe, bool &ne,
                                                 const u8 *oldrow,
                                                 const u8 *newrow, u32 ovb) {
  bool differ = false, new_first = false;
  if (oe && ne) {
    u32 word = 0;
    for (u32 c = 0; c < ovb; c++) {
      u8 a = oldrow[c], b = newrow[c];
      if (a != b && (!differ || (c >> 3) == word)) {
        differ = true;
        word = c >> 3;
        new_first = b < a;
      }
    }
    if (!differ) oe = ne = false;
  }
  return new_first;
}

// Emit the retraction of the old row and the assertion of the new one.
// Every lane of the wave calls this once per iteration: ONE wave-aggregated
// output reservation (per-row atomicAdds on the shared counter serialized
// within each wave — same cure as the probe queues).
//
// Ordered form (gcount != nullptr; single-time pushes): no
// reservation. Group g of the slice writes its 0, 1 or 2 rows to slots 2g
// and 2g + 1 of the (staging) columns and their number to gcount[g]; of two
// rows the one whose val comes first in the canonical val order goes first
// (new_first, from cancel_unchanged).
// Groups are in key order, so compacting the slots in group order
// (k_compact_pairs) yields the consolidated form with no sort.
__device__ __forceinline__ void emit_old_new(
    bool oe, bool ne, const u64 *key, u32 kw, const u8 *oldrow,
    const u8 *newrow, u32 ovb, u64 t, u32 lane, u64 *okeys, u8 *ovals,
    u64 *otimes, i64 *odiffs, unsigned long long *ocount, u32 *gcount,
    u64 g, bool live, bool new_first) {
  u32 c = (oe ? 1u : 0u) + (ne ? 1u : 0u);
  u64 o;
  if (gcount) {
    if (!live) return;
    gcount[g] = c;
    o = 2 * g;
  } else {
    o = wave_reserve(ocount, c, lane);
    new_first = false;  // the sort behind this form orders the rows
  }
  if (oe) {
    u64 at = o + (new_first ? 1 : 0);
    for (u32 w = 0; w < kw; w++) okeys[at * kw + w] = key[w];
    for (u32 cb = 0; cb < ovb; cb++) ovals[at * ovb + cb] = oldrow[cb];
    otimes[at] = t;
    odiffs[at] = -1;
  }
  if (ne) {
    u64 at = o + (oe && !new_first ? 1 : 0);
    for (u32 w = 0; w < kw; w++) okeys[at * kw + w] = key[w];
    for (u32 cb = 0; cb < ovb; cb++) ovals[at * ovb + cb] = newrow[cb];
    otimes[at] = t;
    odiffs[at] = 1;
  }
}

// Compaction of the ordered emit: group g's gcount[g] rows move from slots
// 2g.. to pos[g].., pos being the exclusive scan of PairCountIn over m + 1
// slots; *ocount receives the total.
struct PairCountIn {
  const u32 *gcount, *gidn;
  u64 m;
  __host__ __device__ u32 operator()(u64 g) const {
    return g < gidn[m - 1] ? gcount[g] : 0u;
  }
};
__global__ void k_compact_pairs(const u64 *skeys, const u8 *svals,
                                const u64 *stimes, const i64 *sdiffs,
                                PairCountIn in, const u32 *pos, u32 kw,
                                u32 vb, u64 *okeys, u8 *ovals, u64 *otimes,
                                i64 *odiffs, unsigned long long *ocount) {
  u64 G = in.gidn[in.m - 1];
  if (blockIdx.x == 0 && threadIdx.x == 0) *ocount = pos[in.m];
  GRID_STRIDE(g, G) {
    u32 c = in.gcount[g];
    for (u32 j = 0; j < c; j++) {
      u64 s = 2 * g + j, o = (u64)pos[g] + j;
      for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = skeys[s * kw + w];
      for (u32 b = 0; b < vb; b++) ovals[o * vb + b] = svals[s * vb + b];
      otimes[o] = stimes[s];
      odiffs[o] = sdiffs[s];
    }
  }
}

// Phase C: one thread per distinct key in a time slice [lo,hi) of updates
// sorted by (time, key). gstart: start row of each key group; emits
// corrections (new minus old finalized rows). Uniform-iteration loop so
// the whole wave reaches emit_old_new together.
__global__ void k_reduce_apply(const u64 *keys, const u8 *vals, u32 kw,
                               u32 vb, const i64 *diffs, const u32 *gstart,
                               const u32 *gidn, u64 hi_row, u64 t,
                               RedState st, const u32 *found,
                               const u32 *miss, const u32 *misspos,
                               const u64 *d_nrows, mz_gpu_reduce_spec spec,
                               u64 *okeys, u8 *ovals, u64 *otimes,
                               i64 *odiffs, unsigned long long *ocount,
                               u32 *gcount /* ordered emit, or nullptr */) {
  u32 na = spec.n_aggs;
  u32 ovb = spec.out.val_bytes;
  u64 G = hi_row ? gidn[hi_row - 1] : 0;
  u64 base = *d_nrows;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (G + stride - 1) / stride;
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 g = start0 + it * stride;
    bool oe = false, ne = false, new_first = false;
    const u64 *key = nullptr;
    u8 oldrow[MZ_GPU_MAX_AGGS * 24], newrow[MZ_GPU_MAX_AGGS * 24];
    if (g < G) {
      u64 lo = gstart[g];
      u64 end = (g + 1 < G) ? gstart[g + 1] : hi_row;
      key = keys + lo * kw;
      u64 idx = miss[g] ? base + misspos[g] : found[g];
      if (idx < st.capacity) {  // overflow flagged by insert
        u64 *row = st.rows + idx * st.stride_w;
        i64 *total_p = (i64 *)(row + kw);
        Acc5 *accs = (Acc5 *)(row + kw + 1);
        // snapshot old
        i64 old_total = *total_p;
        Acc5 old_a[MZ_GPU_MAX_AGGS];
        for (u32 a = 0; a < na; a++) old_a[a] = accs[a];
        for (u64 r = lo; r < end; r++) {
          i64 d = diffs[r];
          const u8 *v = vals + r * vb;
          for (u32 a = 0; a < na; a++)
            acc_fold(accs[a], d_datum_to_acc(spec.aggs[a], v), d);
          *total_p = wadd(*total_p, d);
        }
        i64 new_total = *total_p;
        auto exists = [&](const Acc5 *as, i64 tot) {
          if (tot != 0) return true;
          for (u32 a = 0; a < na; a++)
            if (acc_nonzero(as[a])) return true;
          return false;
        };
        oe = exists(old_a, old_total);
        ne = exists(accs, new_total);
        if (oe)
          for (u32 a = 0; a < na; a++)
            d_finalize(spec.aggs[a], old_a[a], old_total, oldrow + 24 * a);
        if (ne)
          for (u32 a = 0; a < na; a++)
            d_finalize(spec.aggs[a], accs[a], new_total, newrow + 24 * a);
        new_first = cancel_unchanged(oe, ne, oldrow, newrow, ovb);
      }
    }
    emit_old_new(oe, ne, key, kw, oldrow, newrow, ovb, t, lane, okeys, ovals,
                 otimes, odiffs, ocount, gcount, g, g < G, new_first);
  }
}

// ---- resident-table compaction/growth (long-running churn: zero-count /
// zero-accum rows are reclaimed and the table doubles when live + incoming
// exceeds capacity; render/threshold.rs erases zeroed entries, reduce's
// trace compaction drops empty accums — same effect, batched).
__global__ void k_row_live_flags(const u64 *rows, u32 stride_w, u32 from,
                                 u64 nrows, u32 *flags) {
  GRID_STRIDE(i, nrows) {
    u32 live = 0;
    for (u32 w = from; w < stride_w; w++) live |= rows[i * stride_w + w] != 0;
    flags[i] = live;
  }
}
__global__ void k_compact_rows(const u64 *rows, u32 stride_w, u64 nrows,
                               const u32 *flags, const u32 *pos,
                               u64 *newrows) {
  GRID_STRIDE(i, nrows) {
    if (!flags[i]) continue;
    u64 j = pos[i];
    for (u32 w = 0; w < stride_w; w++)
      newrows[j * stride_w + w] = rows[i * stride_w + w];
  }
}
__global__ void k_rehash_rows(const u64 *rows, u32 stride_w, u32 kw, u64 n,
                              u64 *hash, u64 slots) {
  GRID_STRIDE(i, n) {
    const u64 *key = rows + i * stride_w;
    u64 h = route_hash(key, kw) & (slots - 1);
    for (;;) {
      u64 *slot = hash + h * (kw + 1);
      unsigned long long prev = atomicCAS((unsigned long long *)(slot + kw),
                                          ~0ull, (unsigned long long)i);
      if (prev == ~0ull) {
        for (u32 w = 0; w < kw; w++) slot[w] = key[w];
        break;
      }
      h = (h + 1) & (slots - 1);
    }
  }
}

// time-change flags over sorted times
// Pack (key words, zero-padded val words) into one combined key row —
// the threshold's grouping key (its "key" is the whole record:
// render/threshold.rs:38-50 iterates (record, count) within a key group;
// state is per (key, record) pair).
__global__ void k_pack_combined(const u64 *keys, u32 kw, const u8 *vals,
                                u32 vb, u64 n, u64 *ck, u32 kw2) {
  GRID_STRIDE(i, n) {
    u64 *dst = ck + i * kw2;
    for (u32 w = 0; w < kw; w++) dst[w] = keys[i * kw + w];
    for (u32 w = kw; w < kw2; w++) {
      u64 word = 0;
      u32 off = (w - kw) * 8;
      u32 m = vb - off < 8 ? vb - off : 8;
      for (u32 b = 0; b < m; b++)
        word |= (u64)vals[i * vb + off + b] << (8 * b);
      dst[w] = word;
    }
  }
}

// Threshold apply: one thread per distinct (key,val) group of a time
// slice. Keeps the wrapping net count resident; emits one correction row
// (the record itself) with diff = pos(new) - pos(old)
// (threshold_local's count.is_positive() filter, threshold.rs:42-47).
__global__ void k_threshold_apply(const u64 *ckeys, u32 kw2,
                                  const i64 *diffs, const u32 *gstart,
                                  const u32 *gidn, u64 m, u64 t,
                                  RedState st, const u32 *found,
                                  const u32 *miss, const u32 *misspos,
                                  const u64 *d_nrows, u32 kw, u32 vb,
                                  u64 *okeys, u8 *ovals, u64 *otimes,
                                  i64 *odiffs, unsigned long long *ocount) {
  u64 G = m ? gidn[m - 1] : 0;
  u64 base = *d_nrows;
  GRID_STRIDE(g, G) {
    u64 lo = gstart[g];
    u64 end = (g + 1 < G) ? gstart[g + 1] : m;
    const u64 *key = ckeys + lo * kw2;
    u64 idx = miss[g] ? base + misspos[g] : found[g];
    if (idx >= st.capacity) continue;  // overflow flagged by insert
    u64 *row = st.rows + idx * st.stride_w;
    i64 *cnt = (i64 *)(row + kw2);
    i64 old = *cnt, nw = old;
    for (u64 r = lo; r < end; r++) nw = wadd(nw, diffs[r]);
    *cnt = nw;
    i64 po = old > 0 ? old : 0, pn = nw > 0 ? nw : 0;
    i64 delta = (i64)((u64)pn - (u64)po);
    if (!delta) continue;
    u64 o = atomicAdd(ocount, 1ull);
    for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = key[w];
    const u8 *vsrc = (const u8 *)(key + kw);
    for (u32 b = 0; b < vb; b++) ovals[o * vb + b] = vsrc[b];
    otimes[o] = t;
    odiffs[o] = delta;
  }
}

// ---- DISTINCT aggregates (AccumulablePlan::distinct_aggrs; the reference
// keeps one distinct (key, datum) arrangement per such aggregate and feeds
// the accumulator its presence changes, reduce.rs:1357-1581). Here: one
// resident pair table per distinct aggregate — a RedState keyed by
// [key words][datum i64] with one wrapping count word, the threshold table
// with kw2 = kw + 1 — and a key stage that folds the pairs' presence deltas
// instead of the raw rows.

// True for the aggregates that take the pair path (MIN/MAX ignore the flag).
__host__ __device__ inline bool agg_is_distinct(const mz_gpu_aggregate &a) {
  return a.distinct && a.func <= MZ_AGG_SUM_F64;
}

// Project (key, datum) of every staged row into a combined key row. A NULL
// datum is neutralized — datum 0 with diff 0 — rather than dropped, so the
// pair stream keeps the input's row count and time slices, and every key
// of a main slice is a key of the pair slice.
__global__ void k_pair_project(const u64 *keys, u32 kw, const u8 *vals,
                               u32 vb, const i64 *diffs, u64 n,
                               mz_gpu_aggregate a, u64 *ck, i64 *pdiffs) {
  GRID_STRIDE(i, n) {
    const u8 *v = vals + i * vb;
    bool null = a.nullable && v[a.off + a.width] != 0;
    u64 *dst = ck + i * (kw + 1);
    for (u32 w = 0; w < kw; w++) dst[w] = keys[i * kw + w];
    dst[kw] = null ? 0 : (u64)d_read_int(v + a.off, a.width);
    pdiffs[i] = null ? 0 : diffs[i];
  }
}

// Pair apply: one thread per (key, datum) group of a time slice. Folds the
// group's diffs into the resident count and leaves the pair's presence
// change (new != 0) - (old != 0) in delta[g]; the key stage reads it in a
// later launch (RedState coherence rule), so no queue and no atomics.
__global__ void k_pair_apply(const i64 *diffs, const u32 *gstart,
                             const u32 *gidn, u64 m, RedState st,
                             const u32 *found, const u32 *miss,
                             const u32 *misspos, const u64 *d_nrows,
                             int *delta) {
  u64 G = m ? gidn[m - 1] : 0;
  u64 base = *d_nrows;
  GRID_STRIDE(g, G) {
    u64 lo = gstart[g];
    u64 end = (g + 1 < G) ? gstart[g + 1] : m;
    u64 idx = miss[g] ? base + misspos[g] : found[g];
    if (idx >= st.capacity) {  // overflow flagged by insert
      delta[g] = 0;
      continue;
    }
    i64 *cnt = (i64 *)(st.rows + idx * st.stride_w + (st.stride_w - 1));
    i64 old = *cnt, nw = old;
    for (u64 r = lo; r < end; r++) nw = wadd(nw, diffs[r]);
    *cnt = nw;
    delta[g] = (nw != 0 ? 1 : 0) - (old != 0 ? 1 : 0);
  }
}

// One distinct aggregate's pair groups of the current slice, as the key
// stage reads them: combined key rows (kw + 1 words, sorted), group starts,
// the inclusive group-id scan (its last entry is the group count) and the
// presence deltas. ck == nullptr: the aggregate is not distinct.
struct PairView {
  const u64 *ck;
  const u32 *gstart;
  const u32 *gidn;
  const int *delta;
};
struct PairViews {
  PairView v[MZ_GPU_MAX_AGGS];
};

// Phase C for operators with distinct aggregates: k_reduce_apply's loop
// and output contract, one thread per changed key. Plain aggregates and
// `total` fold the key's input rows; a distinct aggregate folds
// datum_to_accumulator(datum) * delta over the key's pair groups, which
// are contiguous and key-ordered like the main slice (lower-bound search;
// an all-NULL key finds only its neutral (key, 0) group, delta 0).
__global__ void __launch_bounds__(BLK)
k_reduce_apply_distinct(const u64 *keys, const u8 *vals, u32 kw, u32 vb,
                        const i64 *diffs, const u32 *gstart,
                        const u32 *gidn, u64 hi_row, u64 t, RedState st,
                        const u32 *found, const u32 *miss,
                        const u32 *misspos, const u64 *d_nrows,
                        mz_gpu_reduce_spec spec, PairViews pvs, u64 *okeys,
                        u8 *ovals, u64 *otimes, i64 *odiffs,
                        unsigned long long *ocount,
                        u32 *gcount /* ordered emit, or nullptr */) {
  u32 na = spec.n_aggs;
  u32 ovb = spec.out.val_bytes;
  u32 kw2 = kw + 1;
  u64 G = hi_row ? gidn[hi_row - 1] : 0;
  u64 base = *d_nrows;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (G + stride - 1) / stride;
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 g = start0 + it * stride;
    bool oe = false, ne = false, new_first = false;
    const u64 *key = nullptr;
    u8 oldrow[MZ_GPU_MAX_AGGS * 24], newrow[MZ_GPU_MAX_AGGS * 24];
    if (g < G) {
      u64 lo = gstart[g];
      u64 end = (g + 1 < G) ? gstart[g + 1] : hi_row;
      key = keys + lo * kw;
      u64 idx = miss[g] ? base + misspos[g] : found[g];
      if (idx < st.capacity) {  // overflow flagged by insert
        u64 *row = st.rows + idx * st.stride_w;
        i64 *total_p = (i64 *)(row + kw);
        Acc5 *accs = (Acc5 *)(row + kw + 1);
        i64 old_total = *total_p, new_total = old_total;
        for (u64 r = lo; r < end; r++) new_total = wadd(new_total, diffs[r]);
        *total_p = new_total;
        oe = old_total != 0;
        ne = new_total != 0;
        for (u32 a = 0; a < na; a++) {
          const mz_gpu_aggregate ag = spec.aggs[a];
          const Acc5 old_a = accs[a];
          Acc5 acc = old_a;
          const PairView pv = pvs.v[a];
          if (pv.ck) {
            // the key's pair groups: [first group with key >= ours, while
            // the key matches)
            u64 Gp = pv.gidn[hi_row - 1];
            u64 l = 0, h = Gp;
            while (l < h) {
              u64 mid = (l + h) >> 1;
              if (d_key_cmp(pv.ck + (u64)pv.gstart[mid] * kw2, key, kw) < 0)
                l = mid + 1;
              else
                h = mid;
            }
            for (u64 p = l; p < Gp; p++) {
              const u64 *pk = pv.ck + (u64)pv.gstart[p] * kw2;
              if (d_key_cmp(pk, key, kw) != 0) break;
              i64 dl = pv.delta[p];
              if (!dl) continue;
              // datum_to_accumulator of a non-null integer datum
              if (ag.func == MZ_AGG_SUM_I64)
                acc.accum += (u128)(i128)(i64)pk[kw] * (u128)(i128)dl;
              acc.nn += (u64)dl;
            }
          } else {
            for (u64 r = lo; r < end; r++)
              acc_fold(acc, d_datum_to_acc(ag, vals + r * vb), diffs[r]);
          }
          accs[a] = acc;
          oe |= acc_nonzero(old_a);
          ne |= acc_nonzero(acc);
          d_finalize(ag, old_a, old_total, oldrow + 24 * a);
          d_finalize(ag, acc, new_total, newrow + 24 * a);
        }
        new_first = cancel_unchanged(oe, ne, oldrow, newrow, ovb);
      }
    }
    emit_old_new(oe, ne, key, kw, oldrow, newrow, ovb, t, lane, okeys, ovals,
                 otimes, odiffs, ocount, gcount, g, g < G, new_first);
  }
}

// ------------------------------------------------------------- topk
// Compact one row per distinct group of a sorted slice (group key list
// for the eval probes).
__global__ void k_gather_group_keys(const u64 *keys, u32 kw,
                                    const u32 *starts, const u32 *gidn,
                                    u64 m, u64 *dg) {
  u64 G = m ? gidn[m - 1] : 0;
  GRID_STRIDE(g, G) {
    for (u32 w = 0; w < kw; w++)
      dg[g * kw + w] = keys[(u64)starts[g] * kw + w];
  }
}

__global__ void k_fill_u64(u64 *p, u64 n, u64 v) { GRID_STRIDE(i, n) p[i] = v; }
__global__ void k_fill_u32(u32 *p, u64 n, u32 v) { GRID_STRIDE(i, n) p[i] = v; }
__global__ void k_fill_u8(u8 *p, u64 n, u8 v) { GRID_STRIDE(i, n) p[i] = v; }
// mins[i] = ~0, maxs[i] = 0 in one launch (k_pass_minmax init)
__global__ void k_init_minmax(u64 *mins, u64 *maxs, u64 n) {
  GRID_STRIDE(i, n) {
    mins[i] = ~0ull;
    maxs[i] = 0;
  }
}

__global__ void k_fill_i64(i64 *p, u64 n, i64 v) { GRID_STRIDE(i, n) p[i] = v; }

__global__ void k_check_pos(const i64 *d, u64 n, u64 *err) {
  GRID_STRIDE(i, n) if (d[i] < 0) *err = 1;
}

// Order-column radix key: signed little-endian int biased to unsigned
// order; descending columns invert (compare_columns restatement,
// top_k.rs:733-739).
__global__ void k_order_sortkey(const u8 *vals, u32 vb, const u32 *perm,
                                u64 *skey, u64 n, u32 off, u32 width,
                                u32 desc) {
  GRID_STRIDE(i, n) {
    const u8 *v = vals + (u64)perm[i] * vb + off;
    u64 raw = 0;
    for (u32 b = 0; b < width; b++) raw |= (u64)v[b] << (8 * b);
    i64 x = width == 8 ? (i64)raw : (i64)(int32_t)(u32)raw;
    u64 s = (u64)x ^ 0x8000000000000000ull;
    skey[i] = desc ? ~s : s;
  }
}

// Kept multiplicity of each ordered row: the overlap of its running
// prefix window [lo,hi) with [offset, offset+limit) (top_k.rs:743-766);
// emit with the given sign (old rows negated, new rows positive).
__global__ void k_topk_kept(const u64 *keys, u32 kw, const u8 *vals, u32 vb,
                            const i64 *diffs, const u64 *pre,
                            const u32 *starts, const u32 *gid, u64 n,
                            u64 off, i64 lim, u64 t, i64 sign, u64 *okeys,
                            u8 *ovals, u64 *otimes, i64 *odiffs,
                            unsigned long long *ocount) {
  GRID_STRIDE(i, n) {
    u32 g = gid[i] - 1;
    u64 s = starts[g];
    u64 base = s ? pre[s - 1] : 0;
    u64 lo = (i == s) ? 0 : pre[i - 1] - base;
    u64 hi = pre[i] - base;
    u64 wlo = lo > off ? lo : off;
    u64 whi = hi;
    if (lim >= 0) {
      u64 cap = off + (u64)lim;
      if (whi > cap) whi = cap;
    }
    if (whi <= wlo) continue;
    u64 o = atomicAdd(ocount, 1ull);
    for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = keys[i * kw + w];
    for (u32 b = 0; b < vb; b++) ovals[o * vb + b] = vals[i * vb + b];
    otimes[o] = t;
    odiffs[o] = sign * (i64)(whi - wlo);
  }
}

// ----------------------------------------------------- window functions
// Per-row evaluation of RowNumber / Rank / DenseRank / LagLead /
// FirstValue / LastValue (src/expr/src/relation/func.rs) over one ordered
// snapshot — the TopK ordering: (key, order columns, canonical val).

// d < 0 is the reference's "Non-positive accumulation" error (err[0]); a
// single multiplicity beyond 2^31 - 1 already exceeds the expansion limit
// (err[1]), and without one the u64 prefix sum cannot wrap.
__global__ void k_window_check(const i64 *d, u64 n, u64 *err) {
  GRID_STRIDE(i, n) {
    if (d[i] < 0) err[0] = 1;
    if (d[i] > 0x7FFFFFFFll) err[1] = 1;
  }
}

struct WinOrder {
  u32 n;
  mz_gpu_order_col c[MZ_GPU_MAX_ORDER];
};

// Peer head flags of the ordered rows: the key or any order column differs
// from the previous row (a partition head is a peer head). hidx = the row's
// own index at a head, 0 elsewhere: its inclusive max-scan is each row's
// peer-start index.
__global__ void k_window_peer_flags(const u64 *keys, u32 kw, const u8 *vals,
                                    u32 vb, WinOrder ord, u64 n, u32 *flags,
                                    u32 *hidx) {
  GRID_STRIDE(i, n) {
    bool neq = i == 0;
    for (u32 w = 0; w < kw && !neq; w++)
      neq = keys[i * kw + w] != keys[(i - 1) * kw + w];
    for (u32 j = 0; j < ord.n && !neq; j++) {
      const u8 *a = vals + i * vb + ord.c[j].off;
      neq = d_read_int(a, ord.c[j].width) != d_read_int(a - vb, ord.c[j].width);
    }
    flags[i] = neq ? 1u : 0u;
    hidx[i] = neq ? (u32)i : 0u;
  }
}

// first index in [lo, hi) whose value exceeds x (hi if none)
template <typename T>
__device__ __forceinline__ u64 d_upper_bound(const T *a, u64 lo, u64 hi, T x) {
  while (lo < hi) {
    u64 mid = (lo + hi) >> 1;
    if (a[mid] > x)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// One ordered snapshot of n >= 1 rows: pre = inclusive scan of the diffs,
// gid / starts = the partition groups, pstart = each row's peer-start row,
// pcum = inclusive count of peer heads.
struct WinSnap {
  const u64 *keys;
  const u8 *vals;
  const u64 *pre;
  const u32 *gid, *starts, *pstart, *pcum;
  u64 n;
};
struct WinFuncs {
  u32 n;
  mz_gpu_window_func f[MZ_GPU_MAX_WFUNCS];
};

// Window aggregates (SUM / COUNT / MIN / MAX over a frame). Sums are exact
// in 128-bit two's complement, two limbs; + and - wrap. A frame's sum is a
// difference of two values of one global (unsegmented) wrapping prefix,
// which is exact whenever the true difference fits: |m x| < 2^94 with the
// multiplicities k_window_check admits, over at most 2^32 rows.
struct U128 {
  u64 lo, hi;
};
struct U128Add {
  __host__ __device__ U128 operator()(const U128 &a, const U128 &b) const {
    U128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u);
    return r;
  }
};
__device__ __forceinline__ U128 d_u128_sub(U128 a, U128 b) {
  U128 r;
  r.lo = a.lo - b.lo;
  r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
  return r;
}
// x * c, x signed and c unsigned
__device__ __forceinline__ U128 d_u128_mul(i64 x, u64 c) {
  U128 r;
  r.lo = (u64)x * c;
  r.hi = __umul64hi((u64)x, c) - (x < 0 ? c : 0);
  return r;
}

// Per ordered row, the scan inputs of one datum: w = m x as 128 bits and
// c = m, both 0 under a NULL. Either output may be absent.
__global__ void k_window_sum_terms(const u8 *vals, u32 vb, const i64 *diffs,
                                   u32 off, u32 width, u32 nullable, u64 n,
                                   U128 *w, u64 *c) {
  GRID_STRIDE(i, n) {
    const u8 *src = vals + i * vb + off;
    const bool nn = !(nullable && src[width] != 0);
    const u64 m = (u64)diffs[i];
    if (w) w[i] = nn ? d_u128_mul(d_read_int(src, (u8)width), m) : U128{0, 0};
    if (c) c[i] = nn ? m : 0;
  }
}

// Per ordered row, the datum for a MIN / MAX scan by partition, the scan's
// identity under a NULL. reverse: row i is written at n - 1 - i with its
// partition id beside it, so that a forward scan is the suffix extremum.
__global__ void k_window_ext_terms(const u8 *vals, u32 vb, const u32 *gid,
                                   u32 off, u32 width, u32 nullable,
                                   int is_max, int reverse, u64 n, i64 *x,
                                   u32 *rgid) {
  GRID_STRIDE(i, n) {
    const u8 *src = vals + i * vb + off;
    const bool nn = !(nullable && src[width] != 0);
    const i64 ident = is_max ? INT64_MIN : INT64_MAX;
    const u64 j = reverse ? n - 1 - i : i;
    x[j] = nn ? d_read_int(src, (u8)width) : ident;
    if (reverse) rgid[j] = gid[i];
  }
}

// What the emit kernel reads per aggregate function, indexed as the spec's
// functions: w = inclusive prefix of m x (SUM), c = inclusive prefix of
// m [non-NULL] (absent for COUNT(*) and a datum that cannot be NULL, where
// it is `pre`), x = MIN / MAX: the extremum of the partition's rows up to
// each row, or with sfx from each row on, stored at n - 1 - row.
struct WinAggs {
  const U128 *w[MZ_GPU_MAX_WFUNCS];
  const u64 *c[MZ_GPU_MAX_WFUNCS];
  const i64 *x[MZ_GPU_MAX_WFUNCS];
  u8 sfx[MZ_GPU_MAX_WFUNCS];
};

// Exclusive position q of the global expanded sequence, base <= q <= the
// partition's end: the row *r of [st, e) holding position q - 1 and the
// number *k >= 1 of its copies before q; q = base is (st, 0).
__device__ __forceinline__ void d_window_pos(const u64 *pre, u64 st, u64 e,
                                             u64 base, u64 q, u64 *r,
                                             u64 *k) {
  if (q == base) {
    *r = st;
    *k = 0;
    return;
  }
  u64 i = d_upper_bound<u64>(pre, st, e, q - 1);
  if (i >= e) i = e - 1;
  *r = i;
  *k = q - (i ? pre[i - 1] : 0);
}

// One aggregate at position p of partition [st, e) (row i, peer start ps):
// the frame as [qa, qb) of the global expanded sequence, qa after ka copies
// of row ra and qb after kb copies of row rb, then differences of the
// prefixes at its two ends. Returns the slot's i64; *nul its null byte.
__device__ __forceinline__ u64 d_window_agg(const WinSnap &s,
                                            const WinAggs &A, u32 f,
                                            const mz_gpu_window_func &fn,
                                            u32 vb, u64 i, u64 st, u64 e,
                                            u64 base, u64 M, u64 p, u64 ps,
                                            u64 *err, u8 *nul) {
  u64 ra = st, ka = 0, qa = base, rb = e - 1, qb = base + M;
  bool empty = false;
  if (fn.frame == MZ_WF_FRAME_TO_CURRENT) {
    rb = d_upper_bound<u32>(s.pstart, i + 1, e, (u32)ps) - 1;
    qb = s.pre[rb];
  } else if (fn.frame == MZ_WF_FRAME_ROWS && !wf_rows_whole(fn)) {
    const u32 sk = wf_start_kind(fn), ek = wf_end_kind(fn);
    i64 a = sk == MZ_WB_UNBOUNDED_PRECEDING ? 0
            : sk == MZ_WB_PRECEDING         ? (i64)p - (i64)fn.offset
            : sk == MZ_WB_CURRENT_ROW       ? (i64)p
                                            : (i64)p + (i64)fn.offset;
    i64 b = ek == MZ_WB_UNBOUNDED_FOLLOWING ? (i64)M - 1
            : ek == MZ_WB_PRECEDING         ? (i64)p - (i64)fn.end_offset
            : ek == MZ_WB_CURRENT_ROW       ? (i64)p
                                            : (i64)p + (i64)fn.end_offset;
    if (a < 0) a = 0;
    if (b > (i64)M - 1) b = (i64)M - 1;
    empty = a > b;
    if (!empty) {
      qa = base + (u64)a;
      qb = base + (u64)b + 1;
      u64 k;
      d_window_pos(s.pre, st, e, base, qa, &ra, &ka);
      d_window_pos(s.pre, st, e, base, qb, &rb, &k);
    }
  }
  const u64 kb = qb - (rb ? s.pre[rb - 1] : 0);
  const u8 *va = s.vals + ra * vb + fn.off, *vbp = s.vals + rb * vb + fn.off;
  const bool nna = !(fn.nullable && va[fn.width] != 0);
  const bool nnb = !(fn.nullable && vbp[fn.width] != 0);
  // the frame's non-NULL datums; every position for COUNT(*)
  u64 cnt = 0;
  if (!empty) {
    const u64 *c = A.c[f];
    if (!c)
      cnt = qb - qa;
    else
      cnt = (rb ? c[rb - 1] : 0) + (nnb ? kb : 0) -
            ((ra ? c[ra - 1] : 0) + (nna ? ka : 0));
  }
  *nul = cnt == 0;
  if (fn.func == MZ_WF_COUNT) return cnt;
  if (cnt == 0) return 0;
  if (fn.func == MZ_WF_SUM) {
    const U128 *w = A.w[f];
    U128 hi = rb ? w[rb - 1] : U128{0, 0}, lo = ra ? w[ra - 1] : U128{0, 0};
    if (nnb) hi = U128Add()(hi, d_u128_mul(d_read_int(vbp, fn.width), kb));
    if (nna) lo = U128Add()(lo, d_u128_mul(d_read_int(va, fn.width), ka));
    const U128 d = d_u128_sub(hi, lo);
    if (d.hi != ((i64)d.lo < 0 ? ~0ull : 0ull)) err[2] = 1;
    return d.lo;
  }
  // MIN / MAX: all copies of a row share a datum
  if (!A.sfx[f]) return (u64)A.x[f][rb];
  const u64 r0 = qa < s.pre[ra] ? ra : ra + 1;  // the row holding qa
  return (u64)A.x[f][s.n - 1 - r0];
}

// One thread per output row o of nout, written at row obase + o with
// diff = sign * (expand ? 1 : the row's multiplicity). expand: o is a
// position of the snapshot's expanded sequence and the source row comes
// from an upper-bound search of pre; otherwise o is the row itself. Old
// and new snapshots write disjoint ranges of one buffer: no atomics, and
// the output position does not depend on scheduling. The val rows of a
// block's tile are built in LDS and stored by the whole block, contiguous.
// AGG: the spec holds an aggregate and A its prefix structures; without,
// the instantiation is the kernel the other specs always ran.
template <bool AGG>
__global__ void __launch_bounds__(BLK)
k_window_emit(WinSnap s, WinFuncs F, WinAggs A, u32 kw, u32 vb, u32 ovb,
              int expand, u64 nout, u64 obase, u64 t, i64 sign, u64 *okeys,
              u8 *ovals, u64 *otimes, i64 *odiffs, u64 *err) {
  __shared__ u8 rows[BLK * WIN_MAX_OVB];
  const u64 G = s.gid[s.n - 1];
  for (u64 tile = (u64)blockIdx.x * BLK; tile < nout;
       tile += (u64)gridDim.x * BLK) {
    const u64 o = tile + threadIdx.x;
    if (o < nout) {
      u64 i = o;
      if (expand) {
        i = d_upper_bound<u64>(s.pre, 0, s.n, o);
        if (i >= s.n) i = s.n - 1;
      }
      const u32 g = s.gid[i] - 1;
      const u64 st = s.starts[g];
      const u64 e = (u64)g + 1 < G ? (u64)s.starts[g + 1] : s.n;
      const u64 base = st ? s.pre[st - 1] : 0;
      const u64 M = s.pre[e - 1] - base;  // the partition's expanded size
      const u64 p = o - base;             // position in it (expand only)
      const u64 ps = s.pstart[i];
      u8 *row = rows + threadIdx.x * ovb;
      const u8 *v = s.vals + i * vb;
      for (u32 b = 0; b < vb; b++) row[b] = v[b];
      u32 w = vb;
      for (u32 f = 0; f < F.n; f++) {
        const mz_gpu_window_func fn = F.f[f];
        u64 x = 0;
        if (fn.func == MZ_WF_ROW_NUMBER) {
          x = p + 1;
        } else if (fn.func == MZ_WF_RANK) {
          x = (ps == st ? 0 : s.pre[ps - 1] - base) + 1;
        } else if (fn.func == MZ_WF_DENSE_RANK) {
          x = (u64)(s.pcum[i] - s.pcum[st]) + 1;
        } else if (AGG && wf_is_agg(fn.func)) {
          u8 nul;
          x = d_window_agg(s, A, f, fn, vb, i, st, e, base, M, p, ps, err,
                           &nul);
          if (fn.func != MZ_WF_COUNT) row[w + 8] = nul;
        } else {
          u64 r = st;  // FIRST_VALUE
          bool have = true;
          if (fn.func == MZ_WF_LAG) {
            have = p >= fn.offset;
            r = have ? d_upper_bound<u64>(s.pre, st, e, base + p - fn.offset)
                     : st;
          } else if (fn.func == MZ_WF_LEAD) {
            have = p + fn.offset < M;
            r = have ? d_upper_bound<u64>(s.pre, st, e, base + p + fn.offset)
                     : st;
          } else if (fn.func == MZ_WF_LAST_VALUE) {
            r = fn.frame == MZ_WF_FRAME_PARTITION
                    ? e - 1
                    : d_upper_bound<u32>(s.pstart, i + 1, e, (u32)ps) - 1;
          }
          if (r >= e) r = e - 1;
          u8 nul;
          if (have) {
            const u8 *src = s.vals + r * vb + fn.off;
            nul = fn.nullable && src[fn.width] != 0;
            if (!nul) x = (u64)d_read_int(src, fn.width);
          } else {
            nul = !fn.has_default;
            if (!nul) x = (u64)fn.dflt;
          }
          row[w + 8] = nul;
        }
        for (u32 b = 0; b < 8; b++) row[w + b] = (u8)(x >> (8 * b));
        w += AGG ? wf_slot_bytes(fn.func)
                 : (fn.func <= MZ_WF_DENSE_RANK ? 8u : 9u);
      }
      for (u32 k = 0; k < kw; k++)
        okeys[(obase + o) * kw + k] = s.keys[i * kw + k];
      otimes[obase + o] = t;
      const u64 m = s.pre[i] - (i ? s.pre[i - 1] : 0);
      odiffs[obase + o] = expand ? sign : sign * (i64)m;
    }
    __syncthreads();
    // the tile's rows are contiguous in the output: bytes up to the first
    // 4-byte boundary, aligned words, then the tail
    const u64 left = nout - tile;
    const u32 nb = (u32)(left < BLK ? left : BLK) * ovb;
    u8 *dst = ovals + (obase + tile) * ovb;
    u32 head = (u32)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > nb) head = nb;
    const u32 nw = (nb - head) / 4;
    for (u32 b = threadIdx.x; b < head; b += BLK) dst[b] = rows[b];
    for (u32 q = threadIdx.x; q < nw; q += BLK) {
      const u8 *sp = rows + head + 4 * q;
      *(u32 *)(dst + head + 4 * q) = (u32)sp[0] | (u32)sp[1] << 8 |
                                     (u32)sp[2] << 16 | (u32)sp[3] << 24;
    }
    for (u32 b = head + 4 * nw + threadIdx.x; b < nb; b += BLK)
      dst[b] = rows[b];
    __syncthreads();
  }
}

__global__ void k_time_flags(const u64 *times, const u32 *perm, u32 *flags,
                             u64 n) {
  GRID_STRIDE(i, n)
  flags[i] = (i == 0 || times[perm[i]] != times[perm[i - 1]]) ? 1u : 0u;
}
__global__ void k_key_flags_sorted(const u64 *keys, u32 kw, const u64 *times,
                                   u32 *flags, u64 n) {
  GRID_STRIDE(i, n) {
    if (i == 0) {
      flags[0] = 1;
      continue;
    }
    bool neq = times[i] != times[i - 1];
    for (u32 w = 0; w < kw && !neq; w++)
      neq |= keys[i * kw + w] != keys[(i - 1) * kw + w];
    flags[i] = neq ? 1u : 0u;
  }
}

// -------------------------------------------------- hierarchical min/max
// build_bucketed + ReductionMonoid restatement (reduce.rs:850-1224,:2273):
// levels of (key, val-hash bucket) arrangements; a changed group's
// extremum is recomputed from the level arrangement (retraction-safe) and
// corrections cascade to the next level.

__global__ void k_bucket_keys(const u64 *keys, u32 kw, const u8 *vals,
                              u64 n, u32 b0, u64 *okeys) {
  GRID_STRIDE(i, n) {
    for (u32 w = 0; w < kw; w++) okeys[i * (kw + 1) + w] = keys[i * kw + w];
    u64 vword;
    memcpy(&vword, vals + i * 8, 8);
    okeys[i * (kw + 1) + kw] = route_hash(&vword, 1) % b0;
  }
}

// per changed group: recompute the extremum over the level arrangement
// (multi-batch val merge with net-diff accumulation), compare with the
// state row, emit corrections keyed for the next level.
__global__ void k_minmax_apply(const u64 *gkeys, u64 G, u32 kw2,
                               BatchList bl, int is_max, RedState st,
                               const u32 *found, const u32 *miss,
                               const u32 *misspos, u64 base, u32 out_kw,
                               u32 bucket_next, u64 t, u64 *okeys, u8 *ovals,
                               u64 *otimes, i64 *odiffs,
                               unsigned long long *ocount) {
  GRID_STRIDE(g, G) {
    const u64 *key = gkeys + g * kw2;
    // per-batch cursors over the key's val range
    u32 cur[12], end[12];
    for (int b = 0; b < bl.n; b++) {
      u64 kvr = hash_lookup_range(bl.b[b].hash, bl.b[b].hash_slots, key,
                                  kw2);
      if (kvr != ~0ull) {
        cur[b] = (u32)kvr;
        end[b] = (u32)(kvr >> 32);
      } else {
        cur[b] = end[b] = 0;
      }
    }
    bool exists = false;
    i64 m = 0;
    for (;;) {
      // smallest current val across batches (vals are 8-byte i64 datums;
      // within-batch order is the canonical LE-u64 order — equality is
      // what matters here, u64 order is a valid merge order)
      bool any = false;
      u64 vmin = 0;
      for (int b = 0; b < bl.n; b++) {
        if (cur[b] >= end[b]) continue;
        u64 v;
        memcpy(&v, bl.b[b].vals + (u64)cur[b] * 8, 8);
        if (!any || v < vmin) vmin = v;
        any = true;
      }
      if (!any) break;
      i64 net = 0;
      for (int b = 0; b < bl.n; b++) {
        while (cur[b] < end[b]) {
          u64 v;
          memcpy(&v, bl.b[b].vals + (u64)cur[b] * 8, 8);
          if (v != vmin) break;
          for (u32 q = bl.b[b].vu_off[cur[b]]; q < bl.b[b].vu_off[cur[b] + 1];
               q++)
            net = wadd(net, bl.b[b].diffs[q]);
          cur[b]++;
        }
      }
      if (net != 0) {
        i64 v = (i64)vmin;
        if (!exists || (is_max ? v > m : v < m)) m = v;
        exists = true;
      }
    }
    // state row: [key kw2][exists][value]
    u64 idx = miss[g] ? base + misspos[g] : found[g];
    u64 *row = st.rows + idx * st.stride_w;
    u64 old_exists = row[kw2];
    i64 old_m = (i64)row[kw2 + 1];
    if ((old_exists != 0) == exists && (!exists || old_m == m)) continue;
    if (old_exists) {
      u64 o = atomicAdd(ocount, 1ull);
      for (u32 w = 0; w < out_kw && w < kw2; w++)
        okeys[o * out_kw + w] = key[w];
      if (out_kw == kw2) okeys[o * out_kw + (kw2 - 1)] = key[kw2 - 1] % bucket_next;
      memcpy(ovals + o * 8, &old_m, 8);
      otimes[o] = t;
      odiffs[o] = -1;
    }
    if (exists) {
      u64 o = atomicAdd(ocount, 1ull);
      for (u32 w = 0; w < out_kw && w < kw2; w++)
        okeys[o * out_kw + w] = key[w];
      if (out_kw == kw2) okeys[o * out_kw + (kw2 - 1)] = key[kw2 - 1] % bucket_next;
      memcpy(ovals + o * 8, &m, 8);
      otimes[o] = t;
      odiffs[o] = 1;
    }
    row[kw2] = exists ? 1 : 0;
    row[kw2 + 1] = (u64)m;
  }
}

// ------------------------------------------------------ collated reduce
// ReducePlan::Collation / build_collation restatement (render/reduce.rs):
// every reduction type maintains its own output ("part"); the stitch keeps
// each key's current part values resident and emits one row per key in the
// SQL aggregate order. Part 0 = the accumulable sub-reduce (absent when
// the spec has no COUNT/SUM), then one part per MIN/MAX aggregate.
//
// Stitch state row (u64 words): [key kw][present-mask][payload], payload =
// each part's current output val at a fixed word offset (accumulable part:
// 3 words per slot; a MIN/MAX part: 1 word). All quantities are whole u64
// words: part vals are 24*k or 8 bytes.
#define COL_MAX_PARTS (MZ_GPU_MAX_AGGS + 1)
#define COL_MAX_PW (3 * MZ_GPU_MAX_AGGS)
struct CollateLayout {
  u32 n_aggs, n_parts;
  u32 W;   // tagged-stream val words (the widest part)
  u32 PW;  // payload words
  u32 part_off[COL_MAX_PARTS], part_len[COL_MAX_PARTS];  // payload words
  u32 slot_src[MZ_GPU_MAX_AGGS];  // payload word offset feeding slot i
  u32 slot_mm[MZ_GPU_MAX_AGGS];   // 1: MIN/MAX slot (one word at [8..16))
};

// MIN/MAX over a column of a wider val: the datum at `off` (4 or 8 bytes,
// signed LE) sign-extended into the 8-byte val column the bucket tree
// takes. Keys, times and diffs are shared with the input.
__global__ void k_project_i64(const u8 *vals, u32 vb, u32 off, u32 width,
                              u64 n, u8 *out) {
  GRID_STRIDE(i, n) {
    i64 x = d_read_int(vals + i * vb + off, (u8)width);
    memcpy(out + i * 8, &x, 8);
  }
}

// Append one part's correction rows to the tagged stream
// (key, part, diff, val zero-padded to W words) at row offset `base`.
__global__ void k_collate_pack(const u64 *pkeys, const u8 *pvals,
                               const i64 *pdiffs, u64 m, u32 kw, u32 plen,
                               u32 part, u32 W, u64 t, u64 base, u64 *okeys,
                               u64 *ovals, u32 *oparts, u64 *otimes,
                               i64 *odiffs) {
  const u64 *pv = (const u64 *)pvals;
  GRID_STRIDE(i, m) {
    u64 o = base + i;
    for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = pkeys[i * kw + w];
    for (u32 w = 0; w < W; w++)
      ovals[o * W + w] = w < plen ? pv[i * plen + w] : 0;
    oparts[o] = part;
    otimes[o] = t;
    odiffs[o] = pdiffs[i];
  }
}

// Stitch one key's row from its payload: accumulable slots are copied
// from part 0, a MIN/MAX slot is its part's word in [8..16) of a zero slot.
__device__ __forceinline__ void d_collate_stitch(const CollateLayout &L,
                                                 const u64 *pay, u64 *row) {
  for (u32 a = 0; a < L.n_aggs; a++) {
    u32 s = L.slot_src[a];
    if (L.slot_mm[a]) {
      row[3 * a] = 0;
      row[3 * a + 1] = pay[s];
      row[3 * a + 2] = 0;
    } else {
      row[3 * a] = pay[s];
      row[3 * a + 1] = pay[s + 1];
      row[3 * a + 2] = pay[s + 2];
    }
  }
}

// Phase C of the stitch upsert (lookup / insert run as k_red_lookup /
// k_red_insert in their own launches — RedState coherence rule): one
// thread per changed key over the key-sorted tagged stream. `perm` maps a
// sorted position to its tagged row; skeys are the keys gathered in
// sorted order. Retractions apply before insertions; a key must end with
// every part present or none (else *d_cerr is set and the key emits
// nothing). Same uniform-iteration loop as k_reduce_apply: every lane,
// including those past G, reaches wave_reserve. Launched with BLK threads
// only: the bound lifts the 128-VGPR budget of the default 1024-thread
// assumption, which spilled the two row buffers' tail to scratch.
__global__ void __launch_bounds__(BLK) k_collate_apply(const u64 *skeys, u32 kw, const u32 *perm,
                                const u32 *parts, const i64 *diffs,
                                const u64 *tvals, const u32 *gstart,
                                const u32 *gidn, u64 R, u64 t, RedState st,
                                const u32 *found, const u32 *miss,
                                const u32 *misspos, const u64 *d_nrows,
                                CollateLayout L, u64 *d_cerr, u64 *okeys,
                                u64 *ovals, u64 *otimes, i64 *odiffs,
                                unsigned long long *ocount) {
  u64 G = R ? gidn[R - 1] : 0;
  u64 base = *d_nrows;
  u32 ow = 3 * L.n_aggs;
  u64 full = (1ull << L.n_parts) - 1;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start0 = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (G + stride - 1) / stride;
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 g = start0 + it * stride;
    bool oe = false, ne = false;
    const u64 *key = nullptr;
    u64 oldrow[COL_MAX_PW], newrow[COL_MAX_PW];
    if (g < G) {
      u64 lo = gstart[g];
      u64 end = (g + 1 < G) ? gstart[g + 1] : R;
      key = skeys + lo * kw;
      u64 idx = miss[g] ? base + misspos[g] : found[g];
      if (idx < st.capacity) {  // overflow flagged by insert
        u64 *row = st.rows + idx * st.stride_w;
        u64 *pay = row + kw + 1;
        u64 old_mask = row[kw], mask = old_mask;
        bool bad = false;
        if (old_mask == full) d_collate_stitch(L, pay, oldrow);
        // retractions first: each must match the stored part payload
        for (u64 r = lo; r < end; r++) {
          u64 j = perm[r];
          i64 d = diffs[j];
          if (d == 1) continue;
          u32 p = parts[j];
          if (d != -1 || p >= L.n_parts || !((mask >> p) & 1)) {
            bad = true;
            continue;
          }
          const u64 *v = tvals + j * L.W;
          bool eq = true;
          for (u32 w = 0; w < L.part_len[p]; w++)
            eq &= v[w] == pay[L.part_off[p] + w];
          if (eq)
            mask &= ~(1ull << p);
          else
            bad = true;
        }
        // then insertions: at most one per part, into a vacated part
        for (u64 r = lo; r < end; r++) {
          u64 j = perm[r];
          if (diffs[j] != 1) continue;
          u32 p = parts[j];
          if (p >= L.n_parts || ((mask >> p) & 1)) {
            bad = true;
            continue;
          }
          const u64 *v = tvals + j * L.W;
          for (u32 w = 0; w < L.part_len[p]; w++)
            pay[L.part_off[p] + w] = v[w];
          mask |= 1ull << p;
        }
        if (mask != 0 && mask != full) bad = true;
        if (mask == 0)  // dead row: reclaimable by kt_compact_grow
          for (u32 w = 0; w < L.PW; w++) pay[w] = 0;
        row[kw] = mask;
        if (bad) {
          *d_cerr = 1;
        } else {
          oe = old_mask == full;
          ne = mask == full;
          if (ne) d_collate_stitch(L, pay, newrow);
          if (oe && ne) {
            bool same = true;
            for (u32 w = 0; w < ow; w++) same &= oldrow[w] == newrow[w];
            if (same) oe = ne = false;
          }
        }
      }
    }
    u32 c = (oe ? 1u : 0u) + (ne ? 1u : 0u);
    u64 o = wave_reserve(ocount, c, lane);
    if (oe) {
      for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = key[w];
      for (u32 w = 0; w < ow; w++) ovals[o * ow + w] = oldrow[w];
      otimes[o] = t;
      odiffs[o] = -1;
      o++;
    }
    if (ne) {
      for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = key[w];
      for (u32 w = 0; w < ow; w++) ovals[o * ow + w] = newrow[w];
      otimes[o] = t;
      odiffs[o] = 1;
    }
  }
}

// ================================================================== host

namespace {

struct Ctx;

struct Alloc {
  void *p = nullptr;
  size_t bytes = 0;
};

struct Scratch {
  // bump arena of device memory, grown on demand, reset per call
  void *base = nullptr;
  size_t cap = 0, used = 0;
  void reset() { used = 0; }
  // fini teardown: the arena is plain hipMalloc memory; without this
  // every context leaked its (pre-grown, multi-GB) arena — a long test
  // session with many contexts ran the device out of memory
  void destroy() {
    if (base) (void)hipFree(base);
    for (void *p : retired) (void)hipFree(p);
    base = nullptr;
    retired.clear();
    cap = used = 0;
  }
  void *get(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    if (used + bytes > cap) {
      size_t ncap = std::max<size_t>(2 * cap, used + bytes + (64u << 20));
      void *nb;
      HIP_CHECK(hipMalloc(&nb, ncap));
      // old allocations in this call remain valid until free; we leak-free
      // the previous arena only when no allocations are outstanding (reset
      // happens at call start, so this is safe at call boundaries). To stay
      // safe mid-call we keep old arenas alive until ctx teardown.
      if (base) retired.push_back(base);
      base = nb;
      cap = ncap;
      // re-bump: prior in-call allocations still point into the retired
      // arena; only new requests come from the new one.
      used = 0;
      if (used + bytes > cap) abort();
    }
    void *p = (char *)base + used;
    used += bytes;
    return p;
  }
  std::vector<void *> retired;
};

}  // namespace

// Flat columns: four owned device arrays with room for n rows (at least
// one), the form consolidation writes and build_batch_core / make_out
// take over.
struct FlatCols {
  u64 *keys = nullptr;
  u8 *vals = nullptr;
  u64 *times = nullptr;
  i64 *diffs = nullptr;
};

struct DevUpdates {
  const u64 *keys;
  const u8 *vals;
  const u64 *times;
  const i64 *diffs;
  u64 n;
  int sorted = 0;  // canonical (key,val,time) ascending (see mz_gpu.h)
  const u32 *val_offs = nullptr;  // VARLEN: [n+1] offsets into vals
};

struct mz_gpu_arr {
  DevSchema schema;
  std::vector<DevBatch> batches;
  u64 logical_compaction = 0;
  u64 physical_compaction = 0;
  u64 upper = 0;
  u64 probe_cap_hint = 0;  // last probe's ceil(matches/row): sizes the
                           // single-walk output queue (k_probe_walk)
  u64 path_cap_hint = 0;   // same, for the fused two-stage path probe
                           // starting at this arrangement (k_probe_path2)
  Ctx *ctx = nullptr;
  // Per-arrangement lane: inserts/merges run on this stream with this
  // scratch arena so independent arrangements' maintenance overlaps;
  // ev_done orders downstream probes after the last lane enqueue,
  // ev_gate orders lane work after the main stream's prior enqueues.
  hipStream_t stream = nullptr;
  struct Scratch *lane_scr = nullptr;
  hipEvent_t ev_done = nullptr, ev_gate = nullptr;
  // probes wait ev_ready, recorded when the probe-visible batch list is
  // final for the step (after install+push, BEFORE a deferred merge is
  // enqueued — the merge must not block the probes it runs under)
  hipEvent_t ev_ready = nullptr;
  // Deferred spine merges run on their OWN stream with their own scratch
  // so they never queue ahead of the lane's insert consolidations;
  // ev_mdone (recorded after the merge's count copy) gates the install.
  hipStream_t mstream = nullptr;
  Scratch *merge_scr = nullptr;
  hipEvent_t ev_mdone = nullptr;
  // deferred insert (arr_insert_async): counts land here asynchronously
  // Cached radix sort plan for the insert lane (churn batches have
  // constant per-batch times and keys from a fixed keyspace, so the
  // column min/max plan repeats every step): sort_updates reuses the
  // cached plan WITHOUT the minmax readback sync and enqueues a
  // device-side validity check instead; a mismatch (flag) triggers a
  // synchronous rebuild at the flush before anything is installed.
  struct SortPlan {
    int valid = 0;
    u32 kw = 0, vb = 0;
    u64 hmin[MAX_PASSES], hmax[MAX_PASSES];
    u64 *dev = nullptr;      // device copy [2 * MAX_PASSES]
    u32 *d_flag = nullptr;   // 1 = this batch's minmax not covered
  } sort_plan;
  struct Pending {
    int active = 0;
    u64 cnt[3] = {0, 0, 0};
    u64 flag[1] = {0};       // host copy of sort_plan.d_flag
    DevUpdates staged;       // inputs retained for the redo path
    DevBatch batch;
    u64 lower = 0;  // batch frontier: a time-filtered probe whose delta
                    // upper <= lower cannot see this batch, so it need
                    // not force the flush (1-deep insert pipelining)
    u64 upper = 0;
    // the insert's consolidated FLAT rows (same order and content as
    // batch.times/diffs, in columns of their own), kept so
    // mz_gpu_arr_flush_take can hand the sorted rows to the delta-path
    // probes without re-sorting or copying
    FlatCols flat;
  } pending;
  // deferred spine merge: the merged batch is computed on the lane while
  // probes keep using the pre-merge batch list (identical logical
  // content); it replaces its inputs at the next flush.
  struct PendingMerge {
    int active = 0;
    size_t from = 0, to = 0;
    u64 cnt[3] = {0, 0, 0};
    DevBatch merged;
  } pending_merge;
};

struct mz_gpu_join {
  mz_gpu_arr *arr1, *arr2;
  mz_gpu_closure cl;
};

// A resident keyed table as an operator holds it: the RedState plus the row
// counter the upsert protocol runs on (kt_* helpers).
// Device-counted tables keep the authoritative count in *d_nrows — bumped
// after each slice's apply, never read back mid-push — and n_rows mirrors
// it from the push's closing readback to decide growth before the next
// push. A host-counted table (minmax levels) has no device words and keeps
// its count in n_rows alone.
// Invariant: st.capacity is a power of two >= 16 and st.slots == 2 *
// capacity, because every probe sequence masks with slots - 1. kt_create_at
// rounds the requested capacity up; kt_compact_grow only doubles.
struct KeyedTable {
  RedState st{};
  u32 kw = 0;              // key words; a hash slot is kw + 1 words
  u64 n_rows = 0;          // host mirror of *d_nrows
  u64 *d_nrows = nullptr;  // device row counter
  u64 *d_err = nullptr;    // device error word(s); [0] = capacity exceeded
  bool owns_ctrs = false;  // d_nrows heads a block this table allocated
};

struct mz_gpu_red {
  mz_gpu_reduce_spec spec;
  // One counter block [key rows][err][pair rows * n_dist]: every table of
  // the operator points into it, and a push reads it back in one copy.
  u64 *d_ctr = nullptr;
  KeyedTable tbl;  // accumulator table: [key kw][total][na * 6 words]
  // DISTINCT aggregates: one resident (key, datum) -> count table each,
  // in spec order of the distinct aggregates (see k_pair_apply)
  u32 n_dist = 0;
  u32 dist_agg[MZ_GPU_MAX_AGGS];  // index into spec.aggs
  KeyedTable ptbl[MZ_GPU_MAX_AGGS];
};

// Threshold operator (render/threshold.rs:34-51): net count per (key,val)
// pair in a resident table keyed by the combined (key-words || val-words)
// row; corrections delta = pos(new) - pos(old).
struct mz_gpu_thr {
  mz_gpu_schema s;
  u32 kw2;  // combined key words: key_words + ceil(val_bytes/8)
  KeyedTable tbl;
};

// TopK operator (top_k.rs:322-418): the operator owns its input
// arrangement (the reference's "Arranged TopK input", :647-656); each push
// evaluates changed groups before and after the slice insert and emits
// new-minus-old kept rows. See include/mz_gpu.h for the semantics note.
struct mz_gpu_topk {
  mz_gpu_topk_spec spec;
  mz_gpu_arr *arr = nullptr;  // owned group-contents arrangement
  u64 *d_err = nullptr;
};

// Window-function operator (ReducePlan::Basic, build_basic_aggregate in
// render/reduce.rs): TopK's shape — an owned arrangement of the partition
// contents, changed partitions evaluated before and after each slice's
// insert — with a per-row function evaluation and a wider output row.
struct mz_gpu_window {
  mz_gpu_window_spec spec;
  mz_gpu_arr *arr = nullptr;  // owned partition-contents arrangement
  u64 *d_err = nullptr;       // [0] negative count, [1] a count > 2^31 - 1,
                              // [2] a SUM outside int64
  bool expand = false;        // ROW_NUMBER / LAG / LEAD / a ROWS aggregate:
                              // one row per copy
  bool has_agg = false;       // SUM / COUNT / MIN / MAX: prefixes are built
  bool has_sum = false;       // [1] fails the push without expansion too
};

namespace {

// Sub-phase profiler (MZ_GPU_PROF=1): HIP event pairs per category,
// summed at mz_gpu_prof_dump. Events are recorded on the ctx stream, so
// sums are device-busy time per section (overlap-free on one stream).
struct Prof {
  bool enabled = false;
  std::map<std::string,
           std::vector<std::pair<hipEvent_t, hipEvent_t>>> cats;
};

struct Ctx {
  hipStream_t stream = nullptr;   // the CURRENT lane's stream (arrangement
                                  // inserts/merges temporarily swap in
                                  // their own — see LaneGuard)
  hipStream_t main_stream = nullptr;
  Scratch *scr = nullptr;         // the current lane's scratch arena
  std::string err;
  Scratch scratch;                // the main lane's arena
  Prof prof;
  std::vector<mz_gpu_arr *> arrs;
  std::vector<mz_gpu_join *> joins;
  std::vector<mz_gpu_red *> reds;
  std::vector<struct mz_gpu_collation *> cols;
  std::vector<struct mz_gpu_temporal *> temporals;
  // pinned staging for small device->host readbacks (pageable-staged
  // async copies cost tens of microseconds each; the step does ~a dozen)
  void *pin = nullptr;
  // probe-kernel timing (for bench roofline): accumulated ns and bytes
  double probe_ms = 0;
  u64 probe_rows = 0, probe_launches = 0;
  u64 probe_pairs = 0, probe_batches = 0, probe_alg_bytes = 0;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  int time_kernels = 0;
};

// Stream-ordered allocation: hipMallocAsync/hipFreeAsync on the ctx
// stream avoid the synchronizing hipMalloc/hipFree (which dominated the
// step time before this change — ~100 allocations per step).
struct ProfScope {
  Ctx *c = nullptr;
  hipEvent_t a = nullptr, b = nullptr;
  const char *name;
  ProfScope(Ctx *ctx, const char *n) : name(n) {
    if (!ctx->prof.enabled) return;
    c = ctx;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, c->stream);
  }
  ~ProfScope() {
    if (!c) return;
    (void)hipEventRecord(b, c->stream);
    c->prof.cats[name].push_back({a, b});
  }
};

#define MZ_PROF_CAT2(a, b) a##b
#define MZ_PROF_CAT(a, b) MZ_PROF_CAT2(a, b)
#define MZ_PROF(ctx, name) ProfScope MZ_PROF_CAT(_ps, __LINE__)(ctx, name)

// Swap the ctx onto an arrangement's lane (stream + scratch) for the
// guard's scope. The lane first waits for everything already enqueued on
// the current stream (probes of earlier batches, prior frees), so lane
// work can never overtake readers of the state it mutates; ev_done is
// recorded on exit for downstream probes to wait on.
struct LaneGuard {
  Ctx *c;
  mz_gpu_arr *a;
  hipStream_t ps;
  Scratch *pscr;
  // gate=false: lane work does NOT wait for the main stream's prior
  // enqueues. Only legal for pipelines that touch exclusively fresh
  // memory (the async-insert consolidation: stage + sort + emit into
  // newly-allocated arrays) — install/merge/free paths MUST gate, since
  // they retire batches that in-flight main-stream probes still read.
  LaneGuard(Ctx *ctx, mz_gpu_arr *arr, bool gate = true) : c(ctx), a(arr) {
    ps = c->stream;
    pscr = c->scr;
    if (!a->stream) {
      HIP_CHECK(hipStreamCreate(&a->stream));
      a->lane_scr = new Scratch();
      // pre-grow AND touch: lane arenas otherwise carve + fault their
      // pages inside the first big merges (KFD zeroes fresh VRAM —
      // measured as a 350ms step on a cold box's first process)
      // 6 GB default: the periodic giant merge expands ~30M+ rows into
      // lane scratch (~3-5 GB at the SF1/1M config); outgrowing the
      // arena mid-run costs a synchronous hipMalloc of KFD-zeroed pages
      // (measured as one 459 ms step at 1M-step ~50). Carving happens
      // here, at arrangement creation (untimed).
      static const u64 LANE_ARENA = [] {
        const char *e = getenv("MZ_GPU_LANE_ARENA_GB");
        return (u64)((e ? atof(e) : 6.0) * (double)(1ull << 30));
      }();
      void *w = a->lane_scr->get(LANE_ARENA);
      (void)hipMemsetAsync(w, 0, LANE_ARENA, a->stream);
      a->lane_scr->reset();
      HIP_CHECK(hipEventCreate(&a->ev_done));
      HIP_CHECK(hipEventCreate(&a->ev_gate));
      HIP_CHECK(hipEventCreate(&a->ev_ready));
      (void)hipEventRecord(a->ev_ready, a->stream);
    }
    if (gate && c->stream != a->stream) {
      (void)hipEventRecord(a->ev_gate, c->stream);
      (void)hipStreamWaitEvent(a->stream, a->ev_gate, 0);
    }
    c->stream = a->stream;
    c->scr = a->lane_scr;
  }
  ~LaneGuard() {
    (void)hipEventRecord(a->ev_done, a->stream);
    c->stream = ps;
    c->scr = pscr;
  }
};

// Swap the ctx onto an arrangement's MERGE stream (own scratch): a
// deferred merge reads only installed, fully-computed batches, so it
// needs no ordering edge at all — it runs concurrently with the lane's
// consolidations AND the main stream's probes. Its install is gated by
// ev_mdone (recorded here at scope exit, after the count copy).
struct MergeGuard {
  Ctx *c;
  mz_gpu_arr *a;
  hipStream_t ps;
  Scratch *pscr;
  MergeGuard(Ctx *ctx, mz_gpu_arr *arr) : c(ctx), a(arr) {
    ps = c->stream;
    pscr = c->scr;
    if (!a->mstream) {
      HIP_CHECK(hipStreamCreate(&a->mstream));
      a->merge_scr = new Scratch();
      HIP_CHECK(hipEventCreate(&a->ev_mdone));
    }
    c->stream = a->mstream;
    c->scr = a->merge_scr;
  }
  ~MergeGuard() {
    (void)hipEventRecord(a->ev_mdone, a->mstream);
    c->stream = ps;
    c->scr = pscr;
  }
};

void *dmalloc(Ctx *c, size_t bytes) {
  void *p = nullptr;
  if (bytes == 0) bytes = 16;
  // Coarse size classes for large blocks: spine merges allocate
  // slightly different multi-hundred-MB sizes every cycle, and an exact
  // pool can never reuse them — each miss carves fresh memory from the
  // driver (tens of ms per big merge). Rounding >16 MB requests to
  // 32 MB multiples makes the classes recur (288 GB HBM absorbs the
  // slack).
  if (bytes > (16u << 20))
    bytes = (bytes + (32u << 20) - 1) & ~((size_t)(32u << 20) - 1);
  HIP_CHECK(hipMallocAsync(&p, bytes, c->stream));
  return p;
}

void dfree(Ctx *c, void *p) {
  if (!p) return;
  hipError_t rc = hipFreeAsync(p, c->stream);
  if (rc != hipSuccess) {
    hipPointerAttribute_t at{};
    hipError_t arc = hipPointerGetAttributes(&at, p);
    fprintf(stderr,
            "dfree FAIL %s ptr=%p attr_rc=%d type=%d device=%d\n",
            hipGetErrorString(rc), p, (int)arc, (int)at.type,
            (int)at.device);
    if (!getenv("MZ_DFREE_SOFT")) abort();
  }
}

template <typename T>
T *dnew(Ctx *c, u64 n) {
  return (T *)dmalloc(c, n * sizeof(T));
}

// Copy small device data into the ctx's pinned staging page and sync;
// the returned pointer is valid until the next d2h_pinned on this ctx.
void *d2h_pinned(Ctx *c, const void *dev, size_t bytes) {
  HIP_CHECK(hipMemcpyAsync(c->pin, dev, bytes, hipMemcpyDeviceToHost,
                           c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  return c->pin;
}

// Kernel-based fills for SEMANTIC device state (hash sentinels, counters,
// zero-padding that later passes read as content). hipMemsetAsync fills
// into a freshly-carved hipMallocAsync block were observed to be silently
// LOST on a process's first operations (virgin-context fault: the reduce
// hash table kept its pre-memset zeros, so lookups aliased distinct keys
// onto one row — isolated round 2). Compute-kernel
// writes share the consuming kernels' ordering and address path and are
// not affected; memsets remain only for page-touch warming where content
// is never read.
static void fill_u64(Ctx *c, u64 *p, u64 n, u64 v) {
  hipLaunchKernelGGL(k_fill_u64, dim3(ngrid(n)), dim3(BLK), 0, c->stream, p,
                     n, v);
}
static void fill_u32(Ctx *c, u32 *p, u64 n, u32 v) {
  hipLaunchKernelGGL(k_fill_u32, dim3(ngrid(n)), dim3(BLK), 0, c->stream, p,
                     n, v);
}
static void fill_u8(Ctx *c, u8 *p, u64 n, u8 v) {
  hipLaunchKernelGGL(k_fill_u8, dim3(ngrid(n)), dim3(BLK), 0, c->stream, p,
                     n, v);
}

u64 exclusive_scan_u32(Ctx *c, const u32 *in, u32 *out, u64 n);

// ---- keyed-table lifecycle (struct KeyedTable; protocol: DESIGN.md §4a)

// Create a table of at least `want` rows of [key kw][payload_w words] whose
// counters live where the caller says: words of an operator-owned block, or
// nullptr for a host-counted table. The request is rounded up to a power of
// two, floor 16 (KeyedTable's capacity invariant): it may come straight from
// an environment knob. The hash is filled with the ~0 sentinel by a kernel
// (never a memset, see fill_u64).
static void kt_create_at(Ctx *c, KeyedTable &T, u32 kw, u32 payload_w,
                         u64 want, u64 *d_nrows, u64 *d_err) {
  u64 cap = 16;
  while (cap < want) cap *= 2;
  T.kw = kw;
  T.n_rows = 0;
  T.d_nrows = d_nrows;
  T.d_err = d_err;
  T.st.slots = 2 * cap;
  T.st.capacity = cap;
  T.st.stride_w = kw + payload_w;
  T.st.hash = dnew<u64>(c, T.st.slots * (kw + 1));
  T.st.rows = dnew<u64>(c, cap * T.st.stride_w);
  fill_u64(c, T.st.hash, T.st.slots * (kw + 1), ~0ull);
}

// Same, with the table's own zeroed counter block [rows][err * n_err].
static void kt_create(Ctx *c, KeyedTable &T, u32 kw, u32 payload_w, u64 cap,
                      u32 n_err = 1) {
  u64 *ctr = dnew<u64>(c, 1 + n_err);
  fill_u64(c, ctr, 1 + n_err, 0);
  kt_create_at(c, T, kw, payload_w, cap, ctr, ctr + 1);
  T.owns_ctrs = true;
}

static void kt_free(Ctx *c, KeyedTable &T) {
  dfree(c, T.st.hash);
  dfree(c, T.st.rows);
  if (T.owns_ctrs) dfree(c, T.d_nrows);
  T = KeyedTable();
}

// Initial capacity: the operator's default unless the env names one (a
// negative or unparsable value asks for the floor; kt_create_at rounds).
static u64 kt_env_cap(const char *env, u64 dflt) {
  const char *e = getenv(env);
  if (!e) return dflt;
  long long v = atoll(e);
  return v > 0 ? (u64)v : 0;
}

// Reclaim dead rows (all payload words zero) and grow the table so `need`
// more rows fit: rebuild rows + hash at the new capacity. Synchronizes.
static void kt_compact_grow(Ctx *c, KeyedTable &T, u64 need) {
  auto &S = (*c->scr);
  RedState &st = T.st;
  u64 n = T.n_rows;
  u32 *flags = (u32 *)S.get(std::max<u64>(n, 1) * 4);
  u32 *pos = (u32 *)S.get((std::max<u64>(n, 1) + 1) * 4);
  u64 live = 0;
  if (n) {
    hipLaunchKernelGGL(k_row_live_flags, dim3(ngrid(n)), dim3(BLK), 0,
                       c->stream, st.rows, st.stride_w, T.kw, n, flags);
    live = exclusive_scan_u32(c, flags, pos, n);  // syncs
  }
  u64 newcap = st.capacity;
  while (live + need > newcap) newcap *= 2;
  u64 slots = 2 * newcap;
  u64 *nrows_arr = dnew<u64>(c, newcap * st.stride_w);
  u64 *nhash = dnew<u64>(c, slots * (T.kw + 1));
  fill_u64(c, nhash, slots * (T.kw + 1), ~0ull);
  if (live) {
    hipLaunchKernelGGL(k_compact_rows, dim3(ngrid(n)), dim3(BLK), 0,
                       c->stream, st.rows, st.stride_w, n, flags, pos,
                       nrows_arr);
    hipLaunchKernelGGL(k_rehash_rows, dim3(ngrid(live)), dim3(BLK), 0,
                       c->stream, nrows_arr, st.stride_w, T.kw, live, nhash,
                       slots);
  }
  dfree(c, st.rows);
  dfree(c, st.hash);
  st.rows = nrows_arr;
  st.hash = nhash;
  st.capacity = newcap;
  st.slots = slots;
  T.n_rows = live;
  fill_u64(c, T.d_nrows, 1, live);
}

// Before a push that can open at most n new rows: growth is decided here,
// from the host mirror, so no push ever overflows in flight.
static void kt_reserve(Ctx *c, KeyedTable &T, u64 n) {
  if (T.n_rows + n > T.st.capacity) kt_compact_grow(c, T, n);
}

// Cached-plan validity: slot s covered iff [min,max] within the cached
// bounds, or both plans see a constant column (cached bits = 0 and the
// new column is constant — the pass is skipped either way, so the
// constant's VALUE is irrelevant; this is what lets single-timestamp
// batches reuse the plan as t advances).
__global__ void k_plan_check(const u64 *dminmax, const u64 *cached,
                             u32 nslots, u32 max_passes, u32 *flag) {
  u32 s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  u64 nmin = dminmax[s], nmax = dminmax[s + max_passes];
  u64 cmin = cached[s], cmax = cached[s + max_passes];
  bool ok = (nmin >= cmin && nmax <= cmax) ||
            (cmin == cmax && nmin == nmax);
  if (!ok) atomicOr(flag, 1u);
}

// composite stable sort: returns perm ordering rows by (key, val, time) —
// or (time, key) when for_reduce (primary time).
// Sort passes use rocprim radix_sort_pairs (AMD-native primitive).
void sort_updates(Ctx *c, const u64 *keys, u32 kw, const u8 *vals, u32 vb,
                  const u64 *times, u64 n, u32 *perm, bool time_major,
                  mz_gpu_arr::SortPlan *plan = nullptr) {
  MZ_PROF(c, "sort_updates");
  auto &S = (*c->scr);
  u64 *skey = (u64 *)S.get(n * 8);
  u64 *skey_out = (u64 *)S.get(n * 8);
  u32 *perm_out = (u32 *)S.get(n * 4);
  void *tmp = nullptr;
  size_t tmp_bytes = 0;
  // Column min/max in one sweep: constant columns need no pass at all and
  // the rest subtract the min and radix-sort only the live bits (end_bit)
  // -- most benchmark columns are narrow (dates, keys, small decimals).
  u32 vwords = time_major ? 0 : (vb + 7) / 8;
  if (1 + vwords + kw > MAX_PASSES) {
    fprintf(stderr, "sort_updates: %u sort columns exceed MAX_PASSES\n",
            1 + vwords + kw);
    abort();
  }
  u64 *dminmax = (u64 *)S.get(2 * MAX_PASSES * 8);
  u64 *dmin = dminmax, *dmax = dminmax + MAX_PASSES;
  hipLaunchKernelGGL(k_init_minmax, dim3(1), dim3(BLK), 0, c->stream, dmin,
                     dmax, MAX_PASSES);
  if (n)
    hipLaunchKernelGGL(k_pass_minmax,
                       dim3(ngrid(n), 1 + vwords + kw), dim3(BLK), 0,
                       c->stream, keys, kw, vals, vb, times, n, vwords, 1,
                       dmin, dmax);
  u64 *hmin, *hmax;
  if (plan && plan->valid && plan->kw == kw && plan->vb == vb &&
      !time_major) {
    // cached plan: enqueue the device validity check, no host sync
    hipLaunchKernelGGL(k_plan_check, dim3(1), dim3(64), 0, c->stream,
                       dminmax, plan->dev, 1 + vwords + kw, MAX_PASSES,
                       plan->d_flag);
    hmin = plan->hmin;
    hmax = plan->hmax;
  } else {
    // one pinned staged copy for both halves (dmin/dmax are contiguous)
    u64 *mm = (u64 *)d2h_pinned(c, dminmax, 2 * MAX_PASSES * 8);
    hmin = mm;
    hmax = mm + MAX_PASSES;
    if (plan && !time_major) {
      // (re)prime the cache from this batch's plan, PADDED by one span
      // on each side of every non-constant column: batches are samples
      // of a fixed population, so the sampled min/max jitters — exact
      // bounds would flag (and synchronously redo) nearly every later
      // batch. Constant columns stay exact (their validity rule is
      // value-independent constancy). One extra covered span costs at
      // most ~2 radix bits per column.
      if (!plan->dev) {
        plan->dev = dnew<u64>(c, 2 * MAX_PASSES);
        plan->d_flag = (u32 *)dmalloc(c, 4);
        fill_u32(c, plan->d_flag, 1, 0);
      }
      for (u32 s = 0; s < MAX_PASSES; s++) {
        u64 lo = hmin[s], hi2 = hmax[s];
        if (lo < hi2) {
          // batches sample a fixed population: extremes jitter by
          // O(span/n); span/8 covers that at ~0.1 extra radix bits
          u64 pad = (hi2 - lo) / 8 + 1;
          lo -= std::min(pad, lo);
          hi2 = (hi2 + pad < hi2) ? ~0ull : hi2 + pad;
        }
        plan->hmin[s] = lo;
        plan->hmax[s] = hi2;
      }
      HIP_CHECK(hipMemcpyAsync(plan->dev, plan->hmin, MAX_PASSES * 8,
                               hipMemcpyHostToDevice, c->stream));
      HIP_CHECK(hipMemcpyAsync(plan->dev + MAX_PASSES, plan->hmax,
                               MAX_PASSES * 8, hipMemcpyHostToDevice,
                               c->stream));
      hmin = plan->hmin;  // pinned page gets reused by later readbacks
      hmax = plan->hmax;
      plan->kw = kw;
      plan->vb = vb;
      plan->valid = 1;
    }
  }
  // pass slot layout from k_pass_minmax: [time][val words][key words]
  struct Pass {
    int kind;  // 0 = time, 1 = val word, 2 = key word
    u32 word;
    u64 sub;
    int bits;
  };
  auto slot_of = [&](int kind, u32 word) -> u32 {
    if (kind == 0) return 0;
    if (kind == 1) return 1 + word;
    return 1 + vwords + word;
  };
  // LSD order: least-significant column first
  std::vector<std::pair<int, u32>> order;
  if (time_major) {
    for (int w = (int)kw - 1; w >= 0; w--) order.push_back({2, (u32)w});
    order.push_back({0, 0});
  } else {
    order.push_back({0, 0});
    for (int w = (int)vwords - 1; w >= 0; w--) order.push_back({1, (u32)w});
    for (int w = (int)kw - 1; w >= 0; w--) order.push_back({2, (u32)w});
  }
  std::vector<Pass> passes;
  for (auto &[kind, word] : order) {
    u32 s = slot_of(kind, word);
    if (n == 0 || hmax[s] <= hmin[s]) continue;  // constant column
    u64 range = hmax[s] - hmin[s];
    passes.push_back({kind, word, hmin[s],
                      64 - (int)__builtin_clzll(range)});
  }
  // Pack consecutive LSD passes into <=64-bit composite chunks: one
  // k_sortkey_comp + one rocprim sort per chunk replaces per-column
  // passes (typical TPC-H columns are 14-30 live bits, so 3-5 columns
  // collapse into 1-2 sorts).
  std::vector<std::vector<Pass>> chunks;
  u32 curbits = 0;
  for (auto &p : passes) {
    if (chunks.empty() || curbits + (u32)p.bits > 64 ||
        chunks.back().size() == MAX_COMP) {
      chunks.push_back({});
      curbits = 0;
    }
    chunks.back().push_back(p);
    curbits += (u32)p.bits;
  }
  // No chunk to sort (every column constant, or n == 0): the identity.
  if (chunks.empty()) {
    if (n)
      hipLaunchKernelGGL(k_iota, dim3(ngrid(n)), dim3(BLK), 0, c->stream,
                         perm, n);
    return;
  }
  // Each sort moves the permutation to the other buffer: start where the
  // chunk count's parity makes the last one land in the caller's. The
  // first sort-key kernel writes the identity there itself.
  if (chunks.size() % 2 == 1) std::swap(perm, perm_out);
  u32 *ident = perm;
  for (auto &ch : chunks) {
    int totbits = 0;
    if (ch.size() == 1) {
      const Pass &p = ch[0];
      totbits = p.bits;
      if (p.kind == 0)
        hipLaunchKernelGGL(k_sortkey_u64, dim3(ngrid(n)), dim3(BLK), 0,
                           c->stream, times, perm, skey, n, p.sub, ident);
      else if (p.kind == 1)
        hipLaunchKernelGGL(k_sortkey_val, dim3(ngrid(n)), dim3(BLK), 0,
                           c->stream, vals, vb, p.word, perm, skey, n,
                           p.sub, ident);
      else
        hipLaunchKernelGGL(k_sortkey_key, dim3(ngrid(n)), dim3(BLK), 0,
                           c->stream, keys, kw, p.word, perm, skey, n,
                           p.sub, ident);
    } else {
      CompSpec sp{};
      sp.n = (u32)ch.size();
      u32 shift = 0;
      for (size_t i2 = 0; i2 < ch.size(); i2++) {
        sp.kind[i2] = (u32)ch[i2].kind;
        sp.word[i2] = ch[i2].word;
        sp.sub[i2] = ch[i2].sub;
        sp.shift[i2] = shift;
        shift += (u32)ch[i2].bits;
      }
      totbits = (int)shift;
      hipLaunchKernelGGL(k_sortkey_comp, dim3(ngrid(n)), dim3(BLK), 0,
                         c->stream, keys, kw, vals, vb, times, perm, skey,
                         n, sp, ident);
    }
    ident = nullptr;
    size_t need = 0;
    (void)rocprim::radix_sort_pairs(nullptr, need, skey, skey_out, perm,
                                    perm_out, (unsigned)n, 0, totbits,
                                    c->stream);
    if (need > tmp_bytes) {
      tmp = S.get(need);
      tmp_bytes = need;
    }
    (void)rocprim::radix_sort_pairs(tmp, tmp_bytes, skey, skey_out, perm,
                                    perm_out, (unsigned)n, 0, totbits,
                                    c->stream);
    std::swap(perm, perm_out);
  }
}

// Bounds-checked scan input: in[i] for i < n, 0 for the padding slot —
// replaces the per-scan device copy + fill (two extra launches and a
// full re-read of the input).
struct ScanPadIn {
  const u32 *in;
  u64 n;
  __host__ __device__ u32 operator()(u64 i) const {
    return i < n ? in[i] : 0u;
  }
};

// enqueue-only exclusive scan (out has n+1 slots; no readback)
void exclusive_scan_u32_ns(Ctx *c, const u32 *in, u32 *out, u64 n) {
  auto &S = (*c->scr);
  auto it = rocprim::make_transform_iterator(
      rocprim::make_counting_iterator<u64>(0), ScanPadIn{in, n});
  size_t need = 0;
  (void)rocprim::exclusive_scan(nullptr, need, it, out, 0u, n + 1,
                                rocprim::plus<u32>(), c->stream);
  void *tmp = S.get(need);
  (void)rocprim::exclusive_scan(tmp, need, it, out, 0u, n + 1,
                                rocprim::plus<u32>(), c->stream);
}

// the same scan plus a synchronising read of the total
u64 exclusive_scan_u32(Ctx *c, const u32 *in, u32 *out, u64 n) {
  exclusive_scan_u32_ns(c, in, out, n);
  return *(u32 *)d2h_pinned(c, out + n, 4);
}

__global__ void k_write_u64(u64 *p, u64 v) { *p = v; }
// bump a device counter by pos[G] (the miss total) — G from gidn[m-1]
__global__ void k_bump_ctr(u64 *ctr, const u32 *pos, const u32 *gidn,
                           u64 m) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    u64 G = m ? gidn[m - 1] : 0;
    *ctr += pos[G];
  }
}

void inclusive_scan_u32(Ctx *c, const u32 *in, u32 *out, u64 n) {
  auto &S = (*c->scr);
  size_t need = 0;
  (void)rocprim::inclusive_scan(nullptr, need, in, out, n, rocprim::plus<u32>(),
                          c->stream);
  void *tmp = S.get(need);
  (void)rocprim::inclusive_scan(tmp, need, in, out, n, rocprim::plus<u32>(),
                          c->stream);
}

void inclusive_scan_u64(Ctx *c, const u64 *in, u64 *out, u64 n) {
  auto &S = (*c->scr);
  size_t need = 0;
  (void)rocprim::inclusive_scan(nullptr, need, in, out, n, rocprim::plus<u64>(),
                          c->stream);
  void *tmp = S.get(need);
  (void)rocprim::inclusive_scan(tmp, need, in, out, n, rocprim::plus<u64>(),
                          c->stream);
}

// Stage updates onto the device (if host) and return device pointers.

static inline bool is_varlen(u32 vb) { return vb == 0xFFFFFFFFu; }

DevUpdates stage_updates(Ctx *c, const mz_gpu_updates *u, u32 kw, u32 vb) {
  DevUpdates d;
  d.n = u->n;
  d.sorted = u->sorted;
  if (u->on_device) {
    d.keys = u->keys;
    d.vals = u->vals;
    d.times = u->times;
    d.diffs = u->diffs;
    d.val_offs = u->val_offs;
    return d;
  }
  auto &S = (*c->scr);
  u64 *k = (u64 *)S.get(u->n * kw * 8);
  u8 *v = nullptr;
  u32 *vo = nullptr;
  if (is_varlen(vb)) {
    u64 bytes = u->n ? u->val_offs[u->n] : 0;
    vo = (u32 *)S.get((u->n + 1) * 4);
    v = (u8 *)S.get(std::max<u64>(bytes, 1));
    HIP_CHECK(hipMemcpyAsync(vo, u->val_offs, (u->n + 1) * 4,
                             hipMemcpyHostToDevice, c->stream));
    if (bytes)
      HIP_CHECK(hipMemcpyAsync(v, u->vals, bytes, hipMemcpyHostToDevice,
                               c->stream));
  } else if (vb) {
    v = (u8 *)S.get(u->n * vb);
    HIP_CHECK(hipMemcpyAsync(v, u->vals, u->n * vb, hipMemcpyHostToDevice,
                             c->stream));
  }
  u64 *t = (u64 *)S.get(u->n * 8);
  i64 *df = (i64 *)S.get(u->n * 8);
  HIP_CHECK(hipMemcpyAsync(k, u->keys, u->n * kw * 8, hipMemcpyHostToDevice,
                           c->stream));
  HIP_CHECK(hipMemcpyAsync(t, u->times, u->n * 8, hipMemcpyHostToDevice,
                           c->stream));
  HIP_CHECK(hipMemcpyAsync(df, u->diffs, u->n * 8, hipMemcpyHostToDevice,
                           c->stream));
  d.keys = k;
  d.vals = v;
  d.val_offs = vo;
  d.times = t;
  d.diffs = df;
  return d;
}

struct OutOwned {
  mz_gpu_out pub_;
  // owned device arrays
  u64 *keys;
  u8 *vals;
  u64 *times;
  i64 *diffs;
};

mz_gpu_out *make_out(u64 *k, u8 *v, u64 *t, i64 *d, u64 n, u32 kw, u32 vb) {
  OutOwned *o = new OutOwned();
  o->keys = k;
  o->vals = v;
  o->times = t;
  o->diffs = d;
  o->pub_ = mz_gpu_out{};  // err fields start empty
  o->pub_.keys = k;
  o->pub_.vals = v;
  o->pub_.times = t;
  o->pub_.diffs = d;
  o->pub_.n = n;
  o->pub_.on_device = 1;
  o->pub_.schema.key_words = kw;
  o->pub_.schema.val_bytes = vb;
  return &o->pub_;
}

mz_gpu_out *make_out_vl(u64 *k, u8 *arena, u32 *voffs, u64 *t, i64 *d,
                        u64 n, u64 bytes, u32 kw) {
  mz_gpu_out *o = make_out(k, arena, t, d, n, kw, 0xFFFFFFFFu);
  o->val_offs = voffs;
  o->val_arena_bytes = bytes;
  return o;
}

// Attach a consolidated error stream to an out-batch (ownership moves).
void out_attach_errs(mz_gpu_out *out, u64 *codes, u64 *times, i64 *diffs,
                     u64 n) {
  out->err_n = n;
  out->err_codes = codes;
  out->err_times = times;
  out->err_diffs = diffs;
}

FlatCols flat_alloc(Ctx *c, u64 n, u32 kw, u32 vb) {
  u64 capn = std::max<u64>(n, 1);
  FlatCols f;
  f.keys = dnew<u64>(c, capn * kw);
  f.vals = (u8 *)dmalloc(c, std::max<u64>(capn * vb, 1));
  f.times = dnew<u64>(c, capn);
  f.diffs = dnew<i64>(c, capn);
  return f;
}
void flat_free(Ctx *c, FlatCols &f) {
  for (void *p : {(void *)f.keys, (void *)f.vals, (void *)f.times,
                  (void *)f.diffs})
    dfree(c, p);
  f = FlatCols();
}
// hand the columns over to an out-batch of n rows
mz_gpu_out *make_out(const FlatCols &f, u64 n, u32 kw, u32 vb) {
  return make_out(f.keys, f.vals, f.times, f.diffs, n, kw, vb);
}

// Group n permuted rows by their head flags and sum each group's diffs
// (wrapping), enqueue-only: starts[g] is the first row of group g, gid the
// inclusive group-id scan, gsum[g] the group's sum, nz[g] whether it
// survives and nzpos the exclusive scan of nz — nzpos[n] is the survivor
// count, left on the device.
struct GroupSums {
  u32 *gid, *starts;
  i64 *gsum;
  u32 *nz, *nzpos;
};
GroupSums group_sum_by_perm(Ctx *c, const u32 *flags, const i64 *diffs,
                            const u32 *perm, u64 n) {
  auto &S = (*c->scr);
  GroupSums g;
  g.gid = (u32 *)S.get(n * 4);
  inclusive_scan_u32(c, flags, g.gid, n);
  g.starts = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_group_starts, dim3(ngrid(n)), dim3(BLK), 0, c->stream,
                     flags, g.gid, g.starts, n);
  // wrapping inclusive prefix of permuted diffs
  u64 *pdiff = (u64 *)S.get(n * 8);
  hipLaunchKernelGGL(k_gather_u64, dim3(ngrid(n)), dim3(BLK), 0, c->stream,
                     (const u64 *)diffs, perm, pdiff, n);
  u64 *pref = (u64 *)S.get(n * 8);
  inclusive_scan_u64(c, pdiff, pref, n);
  g.gsum = (i64 *)S.get(n * 8);
  g.nz = (u32 *)S.get((n + 1) * 4);
  hipLaunchKernelGGL(k_group_sums, dim3(ngrid(n)), dim3(BLK), 0, c->stream,
                     g.starts, g.gid, n, pref, g.gsum, g.nz);
  g.nzpos = (u32 *)S.get((n + 1) * 4);
  exclusive_scan_u32_ns(c, g.nz, g.nzpos, n);
  return g;
}

// Enqueue-only consolidation given a ready ordering permutation (group +
// sum + compact) into CAPACITY-sized outputs (in.n rows); dcounts[0]
// receives the consolidated row count on device. times2/diffs2, when given,
// receive a second copy of those two columns (the flush_take hand-off).
void consolidate_with_perm(Ctx *c, u32 kw, u32 vb, DevUpdates in,
                           const u32 *perm, const FlatCols &o, u64 *dcounts,
                           u64 *times2 = nullptr, i64 *diffs2 = nullptr) {
  auto &S = (*c->scr);
  u64 n = in.n;
  if (n == 0) {
    fill_u64(c, dcounts, 1, 0);
    return;
  }
  SegSum *hd = (SegSum *)S.get(n * sizeof(SegSum));
  hipLaunchKernelGGL(k_head_diff, dim3(ngrid(n)), dim3(BLK), 0, c->stream,
                     in.keys, kw, in.vals, vb, in.times, in.diffs, perm, hd,
                     n);
  SegSum *seg = (SegSum *)S.get(n * sizeof(SegSum));
  size_t need = 0;
  (void)rocprim::inclusive_scan(nullptr, need, hd, seg, n, SegSumOp(),
                                c->stream);
  void *tmp = S.get(need);
  (void)rocprim::inclusive_scan(tmp, need, hd, seg, n, SegSumOp(),
                                c->stream);
  SurvivorIn sv{hd, seg, n};
  u32 *pos = (u32 *)S.get((n + 1) * 4);
  auto it = rocprim::make_transform_iterator(
      rocprim::make_counting_iterator<u64>(0), sv);
  need = 0;
  (void)rocprim::exclusive_scan(nullptr, need, it, pos, 0u, n + 1,
                                rocprim::plus<u32>(), c->stream);
  tmp = S.get(need);
  (void)rocprim::exclusive_scan(tmp, need, it, pos, 0u, n + 1,
                                rocprim::plus<u32>(), c->stream);
  hipLaunchKernelGGL(k_emit_survivors, dim3(ngrid(n)), dim3(BLK), 0,
                     c->stream, in.keys, kw, in.vals, vb, in.times, perm, sv,
                     pos, o.keys, o.vals, o.times, o.diffs, times2, diffs2,
                     dcounts);
}

// Core consolidation: sort + group + sum + compact, enqueue-only but for
// the column-min/max read inside sort_updates (none with a cached plan).
void consolidate_core(Ctx *c, u32 kw, u32 vb, DevUpdates in,
                      const FlatCols &o, u64 *dcounts,
                      mz_gpu_arr::SortPlan *plan = nullptr,
                      u64 *times2 = nullptr, i64 *diffs2 = nullptr) {
  MZ_PROF(c, "consolidate_core");
  auto &S = (*c->scr);
  u64 n = in.n;
  if (n == 0) {
    fill_u64(c, dcounts, 1, 0);
    return;
  }
  u32 *perm = (u32 *)S.get(n * 4);
  sort_updates(c, in.keys, kw, in.vals, vb, in.times, n, perm, false,
               plan);
  consolidate_with_perm(c, kw, vb, in, perm, o, dcounts, times2, diffs2);
}

// Synchronous wrapper (ABI-level mz_gpu_consolidate and the consolidated
// probe outputs): returns owned capacity-sized arrays + the exact count.
FlatCols consolidate_dev(Ctx *c, u32 kw, u32 vb, DevUpdates in, u64 *out_n) {
  FlatCols o = flat_alloc(c, in.n, kw, vb);
  u64 *dcounts = (u64 *)(*c->scr).get(3 * 8);
  consolidate_core(c, kw, vb, in, o, dcounts);
  *out_n = *(u64 *)d2h_pinned(c, dcounts, 8);
  return o;
}

// ---- keyed-table push protocol. Every operator with a
// resident table runs, per time slice of its sorted input: group_sorted,
// kt_upsert, its own apply kernel, kt_commit. All scratch comes from
// *c->scr at call time, so the helpers follow a ScrGuard.

mz_gpu_out *empty_out(Ctx *c, u32 kw, u32 vb) {
  return make_out(dnew<u64>(c, 1), (u8 *)dmalloc(c, 1), dnew<u64>(c, 1),
                  dnew<i64>(c, 1), 0, kw, vb);
}

// the varlen empty result: zero rows, val_offs = [0]
mz_gpu_out *empty_out_vl(Ctx *c, u32 kw) {
  mz_gpu_out *o = make_out_vl(dnew<u64>(c, 1), (u8 *)dmalloc(c, 1),
                              dnew<u32>(c, 1), dnew<u64>(c, 1),
                              dnew<i64>(c, 1), 0, 0, kw);
  fill_u32(c, o->val_offs, 1, 0);
  return o;
}

// Key groups of a slice of m rows sorted by (time, key): gid is the
// inclusive group-id scan (gid[m-1] = the group count, which stays on the
// device), starts[g] the first row of group g.
struct Groups {
  u32 *gid, *starts;
};
Groups group_sorted(Ctx *c, const u64 *keys, u32 kw, const u64 *times,
                    u64 m) {
  auto &S = (*c->scr);
  u32 *flags = (u32 *)S.get(m * 4);
  Groups g{(u32 *)S.get(m * 4), (u32 *)S.get(m * 4)};
  hipLaunchKernelGGL(k_key_flags_sorted, dim3(ngrid(m)), dim3(BLK), 0,
                     c->stream, keys, kw, times, flags, m);
  inclusive_scan_u32(c, flags, g.gid, m);
  hipLaunchKernelGGL(k_group_starts, dim3(ngrid(m)), dim3(BLK), 0, c->stream,
                     flags, g.gid, g.starts, m);
  return g;
}

// Phases A and B of the upsert, as two launches (RedState coherence rule):
// look every group's key up, then insert the misses at row *d_nrows + miss
// rank. The caller's apply kernel is phase C — a third launch, resolving
// rows with the same rule — and kt_commit follows it.
struct Upsert {
  u32 *found, *miss, *misspos;
};
Upsert kt_upsert(Ctx *c, const KeyedTable &T, const u64 *keys, Groups g,
                 u64 m) {
  auto &S = (*c->scr);
  Upsert u{(u32 *)S.get(m * 4), (u32 *)S.get(m * 4),
           (u32 *)S.get((m + 1) * 4)};
  hipLaunchKernelGGL(k_red_lookup, dim3(ngrid(m)), dim3(BLK), 0, c->stream,
                     keys, T.kw, g.starts, 0, g.gid, m, T.st, u.found,
                     u.miss);
  exclusive_scan_u32_ns(c, u.miss, u.misspos, m);
  hipLaunchKernelGGL(k_red_insert, dim3(ngrid(m)), dim3(BLK), 0, c->stream,
                     keys, T.kw, g.starts, 0, g.gid, m, u.miss, u.misspos, 0,
                     T.d_nrows, T.d_err, T.st);
  return u;
}

// After the apply kernel: the inserted rows join the count.
void kt_commit(Ctx *c, const KeyedTable &T, Upsert u, Groups g, u64 m) {
  hipLaunchKernelGGL(k_bump_ctr, dim3(1), dim3(1), 0, c->stream, T.d_nrows,
                     u.misspos, g.gid, m);
}

// Time slices [lo, hi) at time t of n rows sorted by time. Boundaries are
// found on the host (few distinct times per batch); a single-timestamp
// batch (upper == lower + 1, the steady-state churn shape) needs neither
// the copy nor the sync.
struct TimeSlice {
  u64 lo, hi, t;
};
std::vector<TimeSlice> time_slices(Ctx *c, const u64 *stm, u64 n, u64 lower,
                                   u64 upper) {
  if (upper <= lower + 1) return {{0, n, lower}};
  std::vector<u64> htimes(n);
  HIP_CHECK(hipMemcpyAsync(htimes.data(), stm, n * 8, hipMemcpyDeviceToHost,
                           c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  std::vector<TimeSlice> slices;
  for (u64 i = 0; i < n;) {
    u64 j = i;
    while (j < n && htimes[j] == htimes[i]) j++;
    slices.push_back({i, j, htimes[i]});
    i = j;
  }
  return slices;
}

// Sort n updates by (time, key) and materialize the sorted columns (vals
// only when vb != 0): in scratch, or in the caller's owned columns `into`
// (room for n rows) when they must outlive a scratch reset.
struct SortedCols {
  u64 *keys;
  u8 *vals;
  u64 *times;
  i64 *diffs;
};
SortedCols sort_gather(Ctx *c, const u64 *keys, u32 kw, const u8 *vals,
                       u32 vb, const u64 *times, const i64 *diffs, u64 n,
                       const FlatCols *into = nullptr) {
  auto &S = (*c->scr);
  u32 *perm = (u32 *)S.get(n * 4);
  sort_updates(c, keys, kw, vals, vb, times, n, perm, true);
  SortedCols s =
      into ? SortedCols{into->keys, into->vals, into->times, into->diffs}
           : SortedCols{(u64 *)S.get(n * kw * 8),
                        (u8 *)S.get(std::max<u64>(n * vb, 1)),
                        (u64 *)S.get(n * 8), (i64 *)S.get(n * 8)};
  hipLaunchKernelGGL(k_gather_updates, dim3(ngrid(n)), dim3(BLK), 0,
                     c->stream, keys, kw, vals, vb, times, diffs, perm, s.keys,
                     s.vals, s.times, s.diffs, n);
  return s;
}

// Stable LSD radix passes over a permutation of n rows, all in scratch.
// Starting from the identity, per sort column (least significant first) the
// caller writes the column's keys in perm() order into skey() and calls
// pass(), which sorts the permutation by the keys' low end_bit bits and
// swaps the buffers. The temp buffer is sized once, for full-word passes
// and for min_bits-wide ones (the narrowest pass the caller will ask for).
struct PermSort {
  Ctx *c;
  u64 n;
  u32 *p, *p_out;
  u64 *k, *k_out;
  size_t tmp_bytes = 0;
  void *tmp;
  PermSort(Ctx *c_, u64 n_, int min_bits = 64) : c(c_), n(n_) {
    auto &S = (*c->scr);
    p = (u32 *)S.get(n * 4);
    p_out = (u32 *)S.get(n * 4);
    k = (u64 *)S.get(n * 8);
    k_out = (u64 *)S.get(n * 8);
    hipLaunchKernelGGL(k_iota, dim3(ngrid(n)), dim3(BLK), 0, c->stream, p, n);
    for (int bits : {64, min_bits}) {
      size_t nb = 0;
      (void)rocprim::radix_sort_pairs(nullptr, nb, k, k_out, p, p_out,
                                      (unsigned)n, 0, bits, c->stream);
      tmp_bytes = std::max(tmp_bytes, nb);
    }
    tmp = S.get(tmp_bytes);
  }
  u64 *skey() const { return k; }
  const u32 *perm() const { return p; }
  void pass(int end_bit = 64) {
    size_t nb = tmp_bytes;
    (void)rocprim::radix_sort_pairs(tmp, nb, k, k_out, p, p_out, (unsigned)n,
                                    0, end_bit, c->stream);
    std::swap(p, p_out);
  }
};

// Correction rows an apply kernel appends through *ocount.
struct CorrBuf {
  u64 *pk;
  u8 *pv;
  u64 *pt;
  i64 *pd;
  unsigned long long *ocount;
  u32 kw, vb;
};
CorrBuf corr_alloc(Ctx *c, u64 cap_rows, u32 kw, u32 vb) {
  CorrBuf b{dnew<u64>(c, cap_rows * kw),
            (u8 *)dmalloc(c, std::max<u64>(cap_rows * vb, 1)),
            dnew<u64>(c, cap_rows),
            dnew<i64>(c, cap_rows),
            (unsigned long long *)(*c->scr).get(8),
            kw,
            vb};
  fill_u64(c, (u64 *)b.ocount, 1, 0);
  return b;
}
void corr_free(Ctx *c, CorrBuf &b) {
  for (void *p : {(void *)b.pk, (void *)b.pv, (void *)b.pt, (void *)b.pd})
    dfree(c, p);
}
// The push's one readback and sync: h[0] = the emitted count, h[1..] =
// n_ctr counter words from d_ctr (the operator's rows and err words). h is
// the pinned page: read it before the next d2h_pinned.
const u64 *corr_read(Ctx *c, const CorrBuf &b, const u64 *d_ctr, u32 n_ctr) {
  u64 *stage = (u64 *)c->pin;
  HIP_CHECK(hipMemcpyAsync(stage, b.ocount, 8, hipMemcpyDeviceToHost,
                           c->stream));
  HIP_CHECK(hipMemcpyAsync(stage + 1, d_ctr, 8 * n_ctr,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  return stage;
}
// Consolidate the emitted rows (the count came back with corr_read:
// sorting the zero-padded capacity dominated this path) and free the
// buffer; the result, or nullptr if the push failed.
mz_gpu_out *corr_finish(Ctx *c, CorrBuf &b, u64 emitted, bool failed) {
  DevUpdates pin{b.pk, b.pv, b.pt, b.pd, emitted};
  u64 Mc;
  FlatCols o = consolidate_dev(c, b.kw, b.vb, pin, &Mc);
  corr_free(c, b);
  if (!failed) return make_out(o, Mc, b.kw, b.vb);
  flat_free(c, o);
  return nullptr;
}

void free_batch(Ctx *c, DevBatch &b) {
  // Batches are probed on the MAIN stream; freeing there (in-order after
  // every probe enqueued so far) is always safe, and lets lane/flush
  // paths retire batches without gating the lane on the main stream.
  hipStream_t ps_stream = c->stream;
  if (c->main_stream) c->stream = c->main_stream;
  for (void *p : {(void *)b.keys, (void *)b.kv_off, (void *)b.vals,
                  (void *)b.vu_off, (void *)b.v_offs, (void *)b.val_key,
                  (void *)b.times, (void *)b.diffs, (void *)b.upd_val,
                  (void *)b.hash})
    dfree(c, p);
  c->stream = ps_stream;
  b = DevBatch();
}

// Enqueue-only batch build over capacity-sized sealed arrays whose actual
// row count lives in dcounts[0]; dcounts[1]/[2] receive n_keys/n_vals.
// Takes ownership of the flat arrays. Caller must sync and fill the
// batch's host-side counts from dcounts.
DevBatch build_batch_core(Ctx *c, u32 kw, u32 vb, u64 *keys, u8 *vals,
                          u64 *times, i64 *diffs, u64 cap, u64 lower,
                          u64 upper, u64 *dcounts, int keep_flat = 0) {
  MZ_PROF(c, "build_batch");
  auto &S = (*c->scr);
  DevBatch b;
  b.lower = lower;
  b.upper = upper;
  if (cap == 0) {
    // placeholders: NEVER adopt the flat arrays here — with keep_flat
    // the caller retains them (flush_take hand-off), and adopting gave
    // the batch a second owner of the same pointers (double free; the
    // recycled VAs then corrupted unrelated batches)
    b.keys = dnew<u64>(c, 1);
    b.vals = (u8 *)dmalloc(c, 1);
    b.times = times;
    b.diffs = diffs;
    b.kv_off = dnew<u32>(c, 1);
    b.vu_off = dnew<u32>(c, 1);
    b.val_key = dnew<u32>(c, 1);
    b.upd_val = dnew<u32>(c, 1);
    fill_u32(c, b.kv_off, 1, 0);
    fill_u32(c, b.vu_off, 1, 0);
    if (!keep_flat) {
      dfree(c, keys);
      dfree(c, vals);
    }
    return b;
  }
  u64 *ids = (u64 *)S.get(cap * 8);
  {
    auto it = rocprim::make_transform_iterator(
        rocprim::make_counting_iterator<u64>(0),
        ChangeFlagsIn{keys, vals, dcounts, kw, vb});
    size_t need = 0;
    (void)rocprim::inclusive_scan(nullptr, need, it, ids, cap,
                                  rocprim::plus<u64>(), c->stream);
    void *tmp = S.get(need);
    (void)rocprim::inclusive_scan(tmp, need, it, ids, cap,
                                  rocprim::plus<u64>(), c->stream);
  }
  b.keys = dnew<u64>(c, cap * kw);
  b.kv_off = dnew<u32>(c, cap + 1);
  b.vals = (u8 *)dmalloc(c, std::max<u64>(cap * vb, 1));
  b.vu_off = dnew<u32>(c, cap + 1);
  b.val_key = dnew<u32>(c, cap);
  b.upd_val = dnew<u32>(c, cap);
  hipLaunchKernelGGL(k_scatter_structure, dim3(ngrid(cap)), dim3(BLK), 0,
                     c->stream, keys, kw, vals, vb, ids, cap, b.keys, b.kv_off, b.vals, b.vu_off, b.val_key,
                     b.upd_val, dcounts);
  b.times = times;
  b.diffs = diffs;
  u64 slots = 16;
  while (slots < 2 * cap) slots <<= 1;
  b.hash_slots = slots;
  b.hash = dnew<u64>(c, slots * (kw + 1));
  // full-line 0xFF fill: lookups check the idx-word sentinel before key
  // compares, so poisoned key words are never read
  fill_u64(c, b.hash, slots * (kw + 1), ~0ull);
  hipLaunchKernelGGL(k_hash_build, dim3(ngrid(cap)), dim3(BLK), 0,
                     c->stream, b.hash, slots, b.keys, kw, b.kv_off,
                     dcounts + 1);
  // flat key/val arrays were re-packed; stream-ordered free is safe
  // (unless the caller keeps them for a flush_take hand-off)
  if (!keep_flat) {
    dfree(c, keys);
    dfree(c, vals);
  }
  return b;
}

// Install, step one: a sealed batch's host-side counts are the three
// dcounts words (n_upds, n_keys, n_vals) once they have been read back.
void set_counts(DevBatch &b, const u64 *cnt) {
  b.n_upds = cnt[0];
  b.n_keys = cnt[1];
  b.n_vals = cnt[2];
}

// Synchronous wrapper for sealed inputs with host-known count.
DevBatch build_batch(Ctx *c, u32 kw, u32 vb, u64 *keys, u8 *vals, u64 *times,
                     i64 *diffs, u64 n, u64 lower, u64 upper) {
  auto &S = (*c->scr);
  u64 *dcounts = (u64 *)S.get(3 * 8);
  hipLaunchKernelGGL(k_write_u64, dim3(1), dim3(1), 0, c->stream, dcounts,
                     n);
  DevBatch b = build_batch_core(c, kw, vb, keys, vals, times, diffs, n,
                                lower, upper, dcounts);
  u64 cnt[3] = {n, 0, 0};
  HIP_CHECK(hipMemcpyAsync(cnt, dcounts, 3 * 8, hipMemcpyDeviceToHost,
                           c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  set_counts(b, cnt);
  return b;
}

// ---- arrangement maintenance protocol: seal, install,
// policy. Everything here runs on the CURRENT lane (c->stream, *c->scr);
// the callers' guards choose it.

// A sealed batch before its install: the batch with its host counts still
// unset, the device words they will be read from (lane scratch), and, when
// the caller asked to keep them, the consolidated flat rows as four columns
// of their own: the flat keys and vals, and a copy of times and diffs that
// the consolidation's emit wrote beside the batch's (which always belong to
// the batch).
struct Sealed {
  DevBatch batch;
  u64 *dcounts = nullptr;
  FlatCols flat;
};

// The seal's tail, enqueue-only: consolidate `in` along a ready ordering
// `perm` into fresh flat columns and build the batch over them. perm ==
// nullptr sorts first (consolidate_core, with the cached plan if given —
// the only way this can synchronise is the min/max read of an unplanned
// sort).
Sealed seal_ordered(Ctx *c, u32 kw, u32 vb, DevUpdates in, const u32 *perm,
                    mz_gpu_arr::SortPlan *plan, u64 lower, u64 upper,
                    int keep_flat) {
  FlatCols o = flat_alloc(c, in.n, kw, vb);
  Sealed s;
  s.dcounts = (u64 *)(*c->scr).get(3 * 8);
  if (keep_flat) {  // sized by capacity: the count is still on the device
    u64 capn = std::max<u64>(in.n, 1);
    s.flat = FlatCols{o.keys, o.vals, dnew<u64>(c, capn), dnew<i64>(c, capn)};
  }
  if (perm)
    consolidate_with_perm(c, kw, vb, in, perm, o, s.dcounts, s.flat.times,
                          s.flat.diffs);
  else
    consolidate_core(c, kw, vb, in, o, s.dcounts, plan, s.flat.times,
                     s.flat.diffs);
  s.batch = build_batch_core(c, kw, vb, o.keys, o.vals, o.times, o.diffs,
                             in.n, lower, upper, s.dcounts, keep_flat);
  return s;
}

// Seal staged updates: order them (identity when the caller vouches for
// canonical order, else the radix sort), then the tail above.
Sealed seal_updates(Ctx *c, u32 kw, u32 vb, DevUpdates d, u64 lower,
                    u64 upper, mz_gpu_arr::SortPlan *plan, int keep_flat) {
  u32 *perm = nullptr;
  if (d.sorted && d.n) {
    // already in canonical order: skip the radix passes, identity perm
    perm = (u32 *)(*c->scr).get(d.n * 4);
    hipLaunchKernelGGL(k_iota, dim3(ngrid(d.n)), dim3(BLK), 0, c->stream,
                       perm, d.n);
  }
  return seal_ordered(c, kw, vb, d, perm, plan, lower, upper, keep_flat);
}

// Install, step two: replace batches [from, to) with their merge. The
// inputs are freed on the MAIN stream (free_batch), in-order after every
// probe of them enqueued so far — no lane gating needed.
void replace_range(Ctx *c, mz_gpu_arr *a, size_t from, size_t to,
                   const DevBatch &merged) {
  for (size_t i = from; i < to; i++) free_batch(c, a->batches[i]);
  a->batches.erase(a->batches.begin() + from, a->batches.begin() + to);
  a->batches.insert(a->batches.begin() + from, merged);
}

// What a merge of batches [from, to) covers: row total and the frontier
// hull (lower 0 for an empty range).
struct RangeHeader {
  u64 total = 0, lower = 0, upper = 0;
};
RangeHeader range_header(const mz_gpu_arr *a, size_t from, size_t to) {
  RangeHeader h;
  u64 lo = UINT64_MAX;
  for (size_t i = from; i < to; i++) {
    h.total += a->batches[i].n_upds;
    lo = std::min(lo, a->batches[i].lower);
    h.upper = std::max(h.upper, a->batches[i].upper);
  }
  h.lower = lo == UINT64_MAX ? 0 : lo;
  return h;
}

void merge_range_vl(Ctx *c, mz_gpu_arr *a, size_t from, size_t to);

// Merge an arrangement's batches [from, to) into one (logical compaction
// applied). Policy is the host's; semantics = concat + advance + consolidate.
// deferred=1: enqueue the merge on the current lane and record it in
// a->pending_merge — the inputs stay in the batch list (probes keep
// using them; the merged batch holds the same logical updates) until
// merge_install replaces them at the next flush.
// (Varlen merges, defined with the varlen consolidation machinery below,
// are always synchronous.)
void merge_range(Ctx *c, mz_gpu_arr *a, size_t from, size_t to,
                 int deferred = 0) {
  if (to - from <= 1) return;
  if (is_varlen(a->schema.vb)) {
    merge_range_vl(c, a, from, to);
    return;
  }
  MZ_PROF(c, "merge_range");
  auto &S = (*c->scr);
  S.reset();
  u32 kw = a->schema.kw, vb = a->schema.vb;
  RangeHeader h = range_header(a, from, to);
  u64 total = h.total;
  u64 *keys = (u64 *)S.get(total * kw * 8);
  u8 *vals = (u8 *)S.get(std::max<u64>(total * vb, 1));
  u64 *times = (u64 *)S.get(total * 8);
  i64 *diffs = (i64 *)S.get(total * 8);
  {
    MZ_PROF(c, "merge_expand");
    u64 base = 0;
    for (size_t i = from; i < to; i++) {
      DevBatch &b = a->batches[i];
      if (b.n_upds)
        hipLaunchKernelGGL(k_expand_batch, dim3(ngrid(b.n_upds)), dim3(BLK),
                           0, c->stream, b, kw, vb, a->logical_compaction,
                           keys, vals, times, diffs, base);
      base += b.n_upds;
    }
  }
  DevUpdates in{keys, vals, times, diffs, total};
  u32 *perm = nullptr;
  if (total) {
    // All inputs are sorted runs (logical-compaction advance is monotone,
    // so expansion preserves order): a merge-path tournament over the
    // expanded index ranges replaces the full radix re-sort — this is the
    // Spine's pairwise merge proper (ColInternalMerger::merge semantics,
    // columnation.rs:653-713), generalized to k runs in ceil(log2 k)
    // passes. First-pass inputs are counting ranges; later passes merge
    // the sorted index arrays with the same row comparator.
    perm = (u32 *)S.get(total * 4);
    {
      MZ_PROF(c, "merge_path");
      RowLess cmp{keys, vals, times, kw, vb};
      u32 *bufB = (u32 *)S.get(total * 4);
      // temp storage scales with input size (merge-path partitions):
      // query an upper bound at (total, total) for both iterator shapes
      size_t tmpsz = 0;
      {
        size_t n1 = 0, n2 = 0;
        auto it0 = rocprim::make_counting_iterator<u32>(0u);
        (void)rocprim::merge(nullptr, n1, it0, it0, perm, (size_t)total,
                             (size_t)total, cmp, c->stream);
        (void)rocprim::merge(nullptr, n2, (const u32 *)perm,
                             (const u32 *)perm, bufB, (size_t)total,
                             (size_t)total, cmp, c->stream);
        tmpsz = std::max(n1, n2);
      }
      void *tmp = S.get(tmpsz);
      // runs as (start, len) index ranges over the expanded arrays
      std::vector<std::pair<u64, u64>> runs;
      u64 base2 = 0;
      for (size_t i = from; i < to; i++) {
        if (a->batches[i].n_upds)
          runs.push_back({base2, a->batches[i].n_upds});
        base2 += a->batches[i].n_upds;
      }
      bool first = true;
      u32 *cur = nullptr;  // buffer holding the current runs' indices
      while (first || runs.size() > 1) {
        u32 *dst = (cur == perm) ? bufB : perm;
        std::vector<std::pair<u64, u64>> next;
        u64 outbase = 0;
        for (size_t i = 0; i + 1 < runs.size(); i += 2) {
          auto [s1, n1] = runs[i];
          auto [s2, n2] = runs[i + 1];
          size_t nb = tmpsz;
          if (first) {
            auto it1 = rocprim::make_counting_iterator<u32>((u32)s1);
            auto it2 = rocprim::make_counting_iterator<u32>((u32)s2);
            (void)rocprim::merge(tmp, nb, it1, it2, dst + outbase,
                                 (size_t)n1, (size_t)n2, cmp, c->stream);
          } else {
            (void)rocprim::merge(tmp, nb, (const u32 *)(cur + s1),
                                 (const u32 *)(cur + s2), dst + outbase,
                                 (size_t)n1, (size_t)n2, cmp, c->stream);
          }
          next.push_back({outbase, n1 + n2});
          outbase += n1 + n2;
        }
        if (runs.size() % 2) {
          auto [s, n1] = runs.back();
          if (first)
            hipLaunchKernelGGL(k_iota_off, dim3(ngrid(n1)), dim3(BLK), 0,
                               c->stream, dst + outbase, n1, (u32)s);
          else
            HIP_CHECK(hipMemcpyAsync(dst + outbase, cur + s, n1 * 4,
                                     hipMemcpyDeviceToDevice, c->stream));
          next.push_back({outbase, n1});
          outbase += n1;
        }
        runs = std::move(next);
        cur = dst;
        first = false;
      }
      if (cur != perm)
        HIP_CHECK(hipMemcpyAsync(perm, cur, total * 4,
                                 hipMemcpyDeviceToDevice, c->stream));
    }
  }
  // the seal's tail over the merged order (an empty range has no order
  // and consolidates to zero rows either way)
  Sealed s = seal_ordered(c, kw, vb, in, perm, nullptr, h.lower, h.upper, 0);
  if (deferred) {
    a->pending_merge.active = 1;
    a->pending_merge.from = from;
    a->pending_merge.to = to;
    a->pending_merge.merged = s.batch;
    HIP_CHECK(hipMemcpyAsync(a->pending_merge.cnt, s.dcounts, 3 * 8,
                             hipMemcpyDeviceToHost, c->stream));
    return;
  }
  u64 cnt[3] = {0, 0, 0};
  HIP_CHECK(hipMemcpyAsync(cnt, s.dcounts, 3 * 8, hipMemcpyDeviceToHost,
                           c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  set_counts(s.batch, cnt);
  replace_range(c, a, from, to, s.batch);
}

// Install a deferred merge whose stream the caller knows to be done (its
// counts have landed in pm.cnt): replace the input range with the merged
// batch.
void merge_install(Ctx *c, mz_gpu_arr *a) {
  auto &pm = a->pending_merge;
  if (!pm.active) return;
  set_counts(pm.merged, pm.cnt);
  replace_range(c, a, pm.from, pm.to, pm.merged);
  pm.active = 0;
}

// Finish a deferred merge now: wait for its stream, then install it.
void merge_finish(Ctx *c, mz_gpu_arr *a) {
  if (!a->pending_merge.active) return;
  if (a->mstream) HIP_CHECK(hipStreamSynchronize(a->mstream));
  merge_install(c, a);
}

}  // namespace

// ================================================================ C ABI


// ================================================= VARLEN arrangements
// Variable-length vals (schema.val_bytes == MZ_GPU_VARLEN): the
// reference's byte-arena row layout (row-spine/src/lib.rs:110-135).
// Vals are arbitrary byte strings (embedded NULs legal) compared
// lexicographically with shorter-prefix-first. Consolidation sorts row
// INDICES with a comparator merge sort (rocprim::merge_sort) instead of
// the radix pipeline — varlen is off the benchmark hot path, and the
// comparator path is exact for any bytes. Batches carry a per-distinct-
// val offset array (v_offs) beside the arena; the key hash index and
// spine policy are unchanged.

__device__ __forceinline__ int d_bytes_cmp(const u8 *a, u32 la,
                                           const u8 *b, u32 lb) {
  u32 m = la < lb ? la : lb;
  for (u32 i = 0; i < m; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  if (la != lb) return la < lb ? -1 : 1;
  return 0;
}

// (key, val, time) canonical order over varlen rows addressed by
// (vstarts, vends) into the arena (for monotone offsets pass offs and
// offs+1).
struct VlRowLess {
  const u64 *keys;
  const u32 *vstarts, *vends;
  const u8 *arena;
  const u64 *times;
  u32 kw;
  __device__ bool operator()(u32 a, u32 b) const {
    for (u32 w = 0; w < kw; w++) {
      i64 x = (i64)keys[(u64)a * kw + w], y = (i64)keys[(u64)b * kw + w];
      if (x != y) return x < y;
    }
    int vc = d_bytes_cmp(arena + vstarts[a], vends[a] - vstarts[a],
                         arena + vstarts[b], vends[b] - vstarts[b]);
    if (vc) return vc < 0;
    return times[a] < times[b];
  }
};

__global__ void k_vl_head_flags(const u64 *keys, u32 kw, const u32 *vstarts,
                                const u32 *vends, const u8 *arena,
                                const u64 *times, const u32 *perm,
                                u32 *flags, u64 n, int with_time) {
  GRID_STRIDE(i, n) {
    if (i == 0) {
      flags[0] = 1;
      continue;
    }
    u32 a = perm[i], b = perm[i - 1];
    bool neq = false;
    for (u32 w = 0; w < kw; w++)
      neq |= keys[(u64)a * kw + w] != keys[(u64)b * kw + w];
    if (!neq)
      neq = d_bytes_cmp(arena + vstarts[a], vends[a] - vstarts[a],
                        arena + vstarts[b], vends[b] - vstarts[b]) != 0;
    if (with_time && !neq) neq = times[a] != times[b];
    flags[i] = neq ? 1u : 0u;
  }
}

// val length of each SURVIVING group's representative row, at its
// compacted output position (zeros elsewhere so the scan is exact)
__global__ void k_vl_survivor_lens(const u32 *starts, const u32 *gid,
                                   const u32 *nz, const u32 *nzpos, u64 n,
                                   const u32 *perm, const u32 *vstarts,
                                   const u32 *vends, u32 *lens) {
  u64 G = n ? gid[n - 1] : 0;
  GRID_STRIDE(g, n) {
    if (g >= G) {
      lens[g] = 0;
      continue;
    }
    if (!nz[g]) continue;  // positions covered by surviving groups only
    u32 r = perm[starts[g]];
    lens[nzpos[g]] = vends[r] - vstarts[r];
  }
}

__global__ void k_vl_emit_consolidated(
    const u64 *keys, u32 kw, const u32 *vstarts, const u32 *vends,
    const u8 *arena, const u64 *times, const u32 *perm, const u32 *starts,
    const i64 *gsum, const u32 *nz, const u32 *nzpos, const u32 *gid,
    u64 n, const u32 *ovoffs /*exclusive [M+1]*/, u64 *okeys, u8 *oarena,
    u64 *otimes, i64 *odiffs) {
  u64 G = n ? gid[n - 1] : 0;
  GRID_STRIDE(g, G) {
    if (!nz[g]) continue;
    u32 o = nzpos[g];
    u32 r = perm[starts[g]];
    for (u32 w = 0; w < kw; w++) okeys[(u64)o * kw + w] = keys[(u64)r * kw + w];
    otimes[o] = times[r];
    odiffs[o] = gsum[g];
    u32 lo = ovoffs[o], len = vends[r] - vstarts[r];
    for (u32 b = 0; b < len; b++) oarena[lo + b] = arena[vstarts[r] + b];
  }
}

__global__ void k_vl_change_flags(const u64 *keys, u32 kw, const u32 *voffs,
                                  const u8 *arena, u32 *kc, u32 *vc, u64 n) {
  GRID_STRIDE(i, n) {
    if (i == 0) {
      kc[0] = 1;
      vc[0] = 1;
      continue;
    }
    bool kneq = false;
    for (u32 w = 0; w < kw; w++)
      kneq |= keys[i * kw + w] != keys[(i - 1) * kw + w];
    bool vneq = kneq ||
        d_bytes_cmp(arena + voffs[i], voffs[i + 1] - voffs[i],
                    arena + voffs[i - 1], voffs[i] - voffs[i - 1]) != 0;
    kc[i] = kneq ? 1u : 0u;
    vc[i] = vneq ? 1u : 0u;
  }
}

__global__ void k_vl_distinct_lens(const u32 *vc, const u32 *voffs, u64 n,
                                   u32 *dl) {
  GRID_STRIDE(i, n) dl[i] = vc[i] ? voffs[i + 1] - voffs[i] : 0;
}

__global__ void k_vl_scatter(const u64 *keys, u32 kw, const u32 *voffs,
                             const u8 *arena, const u32 *kc, const u32 *vc,
                             const u32 *kid, const u32 *vid,
                             const u32 *apos /*inclusive scan of dl*/,
                             u64 n, u64 n_keys, u64 n_vals, u64 abytes,
                             u64 *bkeys, u32 *kv_off, u32 *b_voffs,
                             u8 *barena, u32 *vu_off, u32 *val_key,
                             u32 *upd_val) {
  GRID_STRIDE(i, n) {
    u32 k = kid[i] - 1, v = vid[i] - 1;
    upd_val[i] = v;
    if (kc[i]) {
      for (u32 w = 0; w < kw; w++) bkeys[(u64)k * kw + w] = keys[i * kw + w];
      kv_off[k] = v;
      if (k == 0) kv_off[n_keys] = (u32)n_vals;
    }
    if (vc[i]) {
      u32 len = voffs[i + 1] - voffs[i];
      u32 dst = apos[i] - len;  // exclusive position
      for (u32 b = 0; b < len; b++) barena[dst + b] = arena[voffs[i] + b];
      b_voffs[v] = dst;
      if (v == 0) b_voffs[n_vals] = (u32)abytes;
      vu_off[v] = (u32)i;
      val_key[v] = k;
      if (v == 0) vu_off[n_vals] = (u32)n;
    }
  }
}

// expansion of a varlen batch back to flat rows: lengths pass + copy pass
__global__ void k_vl_expand_lens(DevBatch b, u32 *lens, u64 base) {
  GRID_STRIDE(i, b.n_upds) {
    u32 v = b.upd_val[i];
    lens[base + i] = b.v_offs[v + 1] - b.v_offs[v];
  }
}
__global__ void k_vl_expand_copy(DevBatch b, u32 kw, u64 frontier,
                                 const u32 *ovoffs /*exclusive*/,
                                 u64 *okeys, u8 *oarena, u64 *otimes,
                                 i64 *odiffs, u64 base) {
  GRID_STRIDE(i, b.n_upds) {
    u32 v = b.upd_val[i];
    u32 k = b.val_key[v];
    u64 o = base + i;
    for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = b.keys[(u64)k * kw + w];
    u64 t = b.times[i];
    otimes[o] = t < frontier ? frontier : t;
    odiffs[o] = b.diffs[i];
    u32 lo = ovoffs[o], src = b.v_offs[v], len = b.v_offs[v + 1] - src;
    for (u32 c = 0; c < len; c++) oarena[lo + c] = b.vals[src + c];
  }
}

namespace {

// consolidated varlen columns (owned device arrays, exact sizes)
struct VlCols {
  u64 *keys = nullptr;
  u32 *voffs = nullptr;  // [n+1] monotone
  u8 *arena = nullptr;
  u64 *times = nullptr;
  i64 *diffs = nullptr;
  u64 n = 0, bytes = 0;
};

// Sort + consolidate varlen rows addressed by (vstarts, vends) into
// canonical (key, val, time) order. Synchronizes.
VlCols consolidate_vl(Ctx *c, u32 kw, const u64 *keys, const u32 *vstarts,
                      const u32 *vends, const u8 *arena, const u64 *times,
                      const i64 *diffs, u64 n) {
  auto &S = (*c->scr);
  VlCols out;
  if (n == 0) {
    out.keys = dnew<u64>(c, 1);
    out.voffs = dnew<u32>(c, 1);
    out.arena = (u8 *)dmalloc(c, 1);
    out.times = dnew<u64>(c, 1);
    out.diffs = dnew<i64>(c, 1);
    fill_u32(c, out.voffs, 1, 0);
    return out;
  }
  u32 *perm = (u32 *)S.get(n * 4);
  u32 *perm_out = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_iota, dim3(ngrid(n)), dim3(BLK), 0, c->stream, perm,
                     n);
  VlRowLess cmp{keys, vstarts, vends, arena, times, kw};
  size_t need = 0;
  (void)rocprim::merge_sort(nullptr, need, perm, perm_out, n, cmp,
                            c->stream);
  void *tmp = S.get(need);
  (void)rocprim::merge_sort(tmp, need, perm, perm_out, n, cmp, c->stream);
  std::swap(perm, perm_out);
  u32 *flags = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_vl_head_flags, dim3(ngrid(n)), dim3(BLK), 0,
                     c->stream, keys, kw, vstarts, vends, arena, times,
                     perm, flags, n, 1);
  GroupSums g = group_sum_by_perm(c, flags, diffs, perm, n);
  u64 M = *(u32 *)d2h_pinned(c, g.nzpos + n, 4);  // syncs
  u32 *lens = (u32 *)S.get((n + 1) * 4);
  hipLaunchKernelGGL(k_vl_survivor_lens, dim3(ngrid(n)), dim3(BLK), 0,
                     c->stream, g.starts, g.gid, g.nz, g.nzpos, n, perm,
                     vstarts, vends, lens);
  u32 *ovoffs = dnew<u32>(c, M + 1);
  u64 bytes = exclusive_scan_u32(c, lens, ovoffs, M);  // syncs; [M+1]
  out.n = M;
  out.bytes = bytes;
  out.keys = dnew<u64>(c, std::max<u64>(M, 1) * kw);
  out.arena = (u8 *)dmalloc(c, std::max<u64>(bytes, 1));
  out.times = dnew<u64>(c, std::max<u64>(M, 1));
  out.diffs = dnew<i64>(c, std::max<u64>(M, 1));
  out.voffs = ovoffs;
  if (M)
    hipLaunchKernelGGL(k_vl_emit_consolidated, dim3(ngrid(n)), dim3(BLK),
                       0, c->stream, keys, kw, vstarts, vends, arena,
                       times, perm, g.starts, g.gsum, g.nz, g.nzpos, g.gid,
                       n, ovoffs, out.keys, out.arena, out.times, out.diffs);
  HIP_CHECK(hipStreamSynchronize(c->stream));
  return out;
}

// Build a sealed varlen batch from consolidated columns (takes ownership
// of times/diffs; copies keys/arena into dedup form and frees them).
DevBatch build_batch_vl(Ctx *c, u32 kw, VlCols &&in, u64 lower, u64 upper) {
  auto &S = (*c->scr);
  DevBatch b;
  b.lower = lower;
  b.upper = upper;
  u64 n = in.n;
  b.n_upds = n;
  if (n == 0) {
    b.keys = dnew<u64>(c, 1);
    b.kv_off = dnew<u32>(c, 1);
    b.vals = (u8 *)dmalloc(c, 1);
    b.vu_off = dnew<u32>(c, 1);
    b.v_offs = dnew<u32>(c, 1);
    b.val_key = dnew<u32>(c, 1);
    b.upd_val = dnew<u32>(c, 1);
    b.times = in.times;
    b.diffs = in.diffs;
    fill_u32(c, b.kv_off, 1, 0);
    fill_u32(c, b.vu_off, 1, 0);
    fill_u32(c, b.v_offs, 1, 0);
    for (void *p : {(void *)in.keys, (void *)in.voffs, (void *)in.arena})
      dfree(c, p);
    return b;
  }
  u32 *kc = (u32 *)S.get(n * 4);
  u32 *vc = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_vl_change_flags, dim3(ngrid(n)), dim3(BLK), 0,
                     c->stream, in.keys, kw, in.voffs, in.arena, kc, vc, n);
  u32 *kid = (u32 *)S.get(n * 4);
  u32 *vid = (u32 *)S.get(n * 4);
  inclusive_scan_u32(c, kc, kid, n);
  inclusive_scan_u32(c, vc, vid, n);
  u32 *dl = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_vl_distinct_lens, dim3(ngrid(n)), dim3(BLK), 0,
                     c->stream, vc, in.voffs, n, dl);
  u32 *apos = (u32 *)S.get(n * 4);
  inclusive_scan_u32(c, dl, apos, n);
  // host-read the three totals in one go
  u32 tails[3];
  HIP_CHECK(hipMemcpyAsync(&tails[0], kid + (n - 1), 4,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipMemcpyAsync(&tails[1], vid + (n - 1), 4,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipMemcpyAsync(&tails[2], apos + (n - 1), 4,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  u64 n_keys = tails[0], n_vals = tails[1], abytes = tails[2];
  b.n_keys = n_keys;
  b.n_vals = n_vals;
  b.keys = dnew<u64>(c, n_keys * kw);
  b.kv_off = dnew<u32>(c, n_keys + 1);
  b.vals = (u8 *)dmalloc(c, std::max<u64>(abytes, 1));
  b.v_offs = dnew<u32>(c, n_vals + 1);
  b.vu_off = dnew<u32>(c, n_vals + 1);
  b.val_key = dnew<u32>(c, n_vals);
  b.upd_val = dnew<u32>(c, n);
  hipLaunchKernelGGL(k_vl_scatter, dim3(ngrid(n)), dim3(BLK), 0, c->stream,
                     in.keys, kw, in.voffs, in.arena, kc, vc, kid, vid,
                     apos, n, n_keys, n_vals, abytes, b.keys, b.kv_off,
                     b.v_offs, b.vals, b.vu_off, b.val_key, b.upd_val);
  b.times = in.times;
  b.diffs = in.diffs;
  u64 slots = 16;
  while (slots < 2 * n_keys) slots <<= 1;
  b.hash_slots = slots;
  b.hash = dnew<u64>(c, slots * (kw + 1));
  fill_u64(c, b.hash, slots * (kw + 1), ~0ull);
  // reuse the fixed-width hash build: it reads keys/kv_off and the key
  // count from a device word
  {
    u64 *dc = (u64 *)S.get(8);
    hipLaunchKernelGGL(k_write_u64, dim3(1), dim3(1), 0, c->stream, dc,
                       n_keys);
    hipLaunchKernelGGL(k_hash_build, dim3(ngrid(std::max<u64>(n_keys, 1))),
                       dim3(BLK), 0, c->stream, b.hash, slots, b.keys, kw,
                       b.kv_off, dc);
  }
  for (void *p : {(void *)in.keys, (void *)in.voffs, (void *)in.arena})
    dfree(c, p);
  return b;
}


// Varlen spine merge: expand the batches to flat rows (logical
// compaction advanced), re-consolidate, re-seal — semantics identical to
// the fixed-width merge (concat + advance + consolidate).
void merge_range_vl(Ctx *c, mz_gpu_arr *a, size_t from, size_t to) {
  auto &S = (*c->scr);
  S.reset();
  u32 kw = a->schema.kw;
  RangeHeader h = range_header(a, from, to);
  u64 total = h.total;
  u64 capn = std::max<u64>(total, 1);
  u64 *keys = (u64 *)S.get(capn * kw * 8);
  u32 *lens = (u32 *)S.get((capn + 1) * 4);
  u64 *times = (u64 *)S.get(capn * 8);
  i64 *diffs = (i64 *)S.get(capn * 8);
  u64 base = 0;
  for (size_t i = from; i < to; i++) {
    DevBatch &b = a->batches[i];
    if (b.n_upds)
      hipLaunchKernelGGL(k_vl_expand_lens, dim3(ngrid(b.n_upds)),
                         dim3(BLK), 0, c->stream, b, lens, base);
    base += b.n_upds;
  }
  u32 *voffs = (u32 *)S.get((capn + 1) * 4);
  u64 bytes = total ? exclusive_scan_u32(c, lens, voffs, total) : 0;
  u8 *arena = (u8 *)S.get(std::max<u64>(bytes, 1));
  base = 0;
  for (size_t i = from; i < to; i++) {
    DevBatch &b = a->batches[i];
    if (b.n_upds)
      hipLaunchKernelGGL(k_vl_expand_copy, dim3(ngrid(b.n_upds)),
                         dim3(BLK), 0, c->stream, b, kw,
                         a->logical_compaction, voffs, keys, arena,
                         times, diffs, base);
    base += b.n_upds;
  }
  VlCols cc = consolidate_vl(c, kw, keys, voffs, voffs + 1, arena, times,
                             diffs, total);
  DevBatch merged = build_batch_vl(c, kw, std::move(cc), h.lower, h.upper);
  HIP_CHECK(hipStreamSynchronize(c->stream));
  replace_range(c, a, from, to, merged);
}

}  // namespace

// Varlen probe: one thread per (delta row, batch); counts rows AND arena
// bytes, reserves both queues per wave, emits key fields + passthrough
// varlen val bytes. The closure must not reference the varlen (lookup)
// side except as the single whole-val passthrough (validated host-side).
// Its second queue is the val arena (bytes), not errors: the same
// reservation (queue_reserve) over ctr[0] rows / ctr[1] bytes.
struct VlQueue {
  u64 cap, bcap;
  unsigned long long *ctr;  // [0] rows, [1] arena bytes
  u64 *okeys;
  u32 *ovstarts, *ovends;
  u8 *oarena;
  u64 *otimes;
  i64 *odiffs;
  __device__ __forceinline__ bool reserve(u32 c, u32 bytes, u32 lane,
                                          u64 *o, u64 *bo) const {
    return queue_reserve(ctr, cap, bcap, c, bytes, lane, o, bo);
  }
};

__global__ void k_probe_vl(DeltaView d, BatchList bl, int mode, int swap,
                           const mz_gpu_closure cl, VlQueue q) {
  u32 okw = cl.out.key_words;
  u64 n = d.n;
  u32 kw = d.kw;
  u64 total = n * (u64)bl.n;
  u64 stride = (u64)gridDim.x * blockDim.x;
  u64 start = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  u64 iters = (total + stride - 1) / stride;
  u32 lane = threadIdx.x & 63;
  for (u64 it = 0; it < iters; it++) {
    u64 idx = start + it * stride;
    bool active = idx < total;
    u64 kvr = ~0ull;
    u32 c = 0, bytes = 0;
    u64 i = 0;
    int bi = 0;
    int cls = 0;
    if (active) {
      i = idx % n;
      bi = (int)(idx / n);
      const DevBatch &b = bl.b[bi];
      const u64 *key = d.keys + i * kw;
      const u8 *dv = d.vals ? d.vals + i * d.vb : nullptr;
      cls = d_closure_apply(&cl, key, swap ? nullptr : dv,
                            swap ? dv : nullptr, nullptr, nullptr);
      if (cls == 1) {
        kvr = hash_lookup_range(b.hash, b.hash_slots, key, kw);
        if (kvr != ~0ull) {
          u64 t = d.times[i];
          for (u32 j = (u32)kvr; j < (u32)(kvr >> 32); j++) {
            u32 len = b.v_offs[j + 1] - b.v_offs[j];
            u32 m = d_time_count(b, bl.allpass[bi], mode, b.vu_off[j],
                                 b.vu_off[j + 1], t);
            c += m;
            bytes += m * len;
          }
        }
      }
    }
    u64 o, bo;
    if (!q.reserve(c, bytes, lane, &o, &bo)) continue;
    const DevBatch &b = bl.b[bi];
    DeltaView::Row r = d.row(i);
    const u64 *key = r.key;
    const u8 *dv = r.val;
    u64 t = r.t;
    i64 d1 = r.d;
    for (u32 j = (u32)kvr; j < (u32)(kvr >> 32); j++) {
      u32 vsrc = b.v_offs[j], len = b.v_offs[j + 1] - vsrc;
      for (u32 u = b.vu_off[j]; u < b.vu_off[j + 1]; u++) {
        // d_time_out written out: calling it costs this kernel 2 VGPRs
        // ("Probe-protocol refactor")
        u64 tout;
        if (bl.allpass[bi]) {
          tout = t;
        } else if (mode == PM_JOIN) {
          u64 t2 = b.times[u];
          tout = t2 > t ? t2 : t;
        } else {
          u64 t2 = b.times[u];
          if (!((mode == PM_HALF_LE) ? (t2 <= t) : (t2 < t))) continue;
          tout = t;
        }
        (void)d_closure_apply(&cl, key, swap ? nullptr : dv,
                              swap ? dv : nullptr, q.okeys + o * okw,
                              (u8 *)(q.okeys + o * okw));
        q.otimes[o] = tout;
        q.odiffs[o] = wmul(d1, b.diffs[u]);
        q.ovstarts[o] = (u32)bo;
        q.ovends[o] = (u32)(bo + len);
        for (u32 cc = 0; cc < len; cc++)
          q.oarena[bo + cc] = b.vals[vsrc + cc];
        o++;
        bo += len;
      }
    }
  }
}

static void arr_flush_impl(Ctx *ctx, mz_gpu_arr *a);
static void arr_insert_vl(Ctx *ctx, mz_gpu_arr *a, const mz_gpu_updates *u);

// ---- probe protocol, host half: the steps every probe
// driver (probe_impl, probe_vl_impl, mz_gpu_halfjoin2) runs, each written
// once.

// Make a lookup arrangement ready to be probed on the ctx stream. A probe
// after insert_async must see the batch (probes of the OLD state precede
// the insert call entirely), and must run after the lookup lane's
// enqueued maintenance. Exception (1-deep insert pipeline): a
// time-filtered probe (le/lt half-join) whose delta times all precede a
// pending batch's lower frontier cannot match any of its rows
// (t2 >= lower >= delta.upper > t1), so the pending insert may keep
// consolidating on its lane while this probe runs — skipping the flush
// (and its lane sync) entirely. (Varlen arrangements never hold a pending
// insert, so they always flush.)
static void probe_prepare(Ctx *ctx, mz_gpu_arr *lk, int mode,
                          u64 delta_upper) {
  bool future_pending = (mode == PM_HALF_LE || mode == PM_HALF_LT) &&
                        lk->pending.active && !lk->pending_merge.active &&
                        lk->pending.lower >= delta_upper;
  if (!future_pending) arr_flush_impl(ctx, lk);
  if (lk->stream) (void)hipStreamWaitEvent(ctx->stream, lk->ev_ready, 0);
}

// Snapshot the probe-visible batches (see BatchList for allpass). A spine
// deeper than the list catches up synchronously first — install any
// deferred merge (its inputs are in the list being merged), then merge
// everything into one batch. Defensive: every insert path already caps
// the spine at 10 batches.
static void build_probe_batchlist(Ctx *ctx, mz_gpu_arr *a, u64 delta_lower,
                                  BatchList &bl) {
  for (;;) {
    bl.n = 0;
    bool fits = true;
    for (auto &b : a->batches) {
      if (b.n_upds == 0) continue;
      if (bl.n >= 12) {
        fits = false;
        break;
      }
      u64 tmax_excl = std::max(b.upper, a->logical_compaction + 1);
      bl.allpass[bl.n] = tmax_excl <= delta_lower ? 1 : 0;
      bl.b[bl.n++] = b;
    }
    if (fits) return;
    merge_finish(ctx, a);
    merge_range(ctx, a, 0, a->batches.size());
  }
}

// Owning host side of the kernels' EmitQueue.
struct ProbeQueue {
  u32 okw, ovb;
  EmitQueue q;
  void alloc(Ctx *c, u64 cap, u64 ecap) {
    q.cap = cap;
    q.ecap = ecap;
    q.okeys = dnew<u64>(c, cap * okw);
    q.ovals = (u8 *)dmalloc(c, std::max<u64>(cap * ovb, 1));
    q.otimes = dnew<u64>(c, cap);
    q.odiffs = dnew<i64>(c, cap);
    q.ecodes = dnew<u64>(c, ecap);
    q.etimes = dnew<u64>(c, ecap);
    q.ediffs = dnew<i64>(c, ecap);
  }
  void free_ok(Ctx *c) {
    for (void *p : {(void *)q.okeys, (void *)q.ovals, (void *)q.otimes,
                    (void *)q.odiffs})
      dfree(c, p);
  }
  void free_errs(Ctx *c) {
    for (void *p : {(void *)q.ecodes, (void *)q.etimes, (void *)q.ediffs})
      dfree(c, p);
  }
  void free(Ctx *c) {
    free_ok(c);
    free_errs(c);
  }
};

// ... and of the varlen probe's VlQueue (rows, arena bytes).
struct VlProbeQueue {
  u32 okw;
  VlQueue q;
  void alloc(Ctx *c, u64 cap, u64 bcap) {
    q.cap = cap;
    q.bcap = bcap;
    q.okeys = dnew<u64>(c, cap * okw);
    q.ovstarts = dnew<u32>(c, cap);
    q.ovends = dnew<u32>(c, cap);
    q.oarena = (u8 *)dmalloc(c, bcap);
    q.otimes = dnew<u64>(c, cap);
    q.odiffs = dnew<i64>(c, cap);
  }
  void free(Ctx *c) {
    for (void *p : {(void *)q.okeys, (void *)q.ovstarts, (void *)q.ovends,
                    (void *)q.oarena, (void *)q.otimes, (void *)q.odiffs})
      dfree(c, p);
  }
};

struct ProbeCounts {
  u64 M, E;  // exact totals of the first / second queue
  u64 I;     // third counter (the fused path's intermediates), else 0
};

// Run one probe: allocate pq at (cap, cap2), zero the nctr counters,
// launch(pq.q), read the counters back. They are exact whether or not
// the queues held them, so on overflow ONE relaunch at the exact counts
// suffices and nothing is read again. With kernel timing on, the (last)
// launch is bracketed by ev_a/ev_b and the call is entered in the probe
// statistics as a probe of n delta rows.
template <class Queue, class Launch>
static ProbeCounts run_probe(Ctx *ctx, Queue &pq, u64 cap, u64 cap2,
                             int nctr, u64 n, Launch launch) {
  unsigned long long *ctr =
      (unsigned long long *)(*ctx->scr).get(8 * nctr);
  pq.q.ctr = ctr;
  pq.alloc(ctx, cap, cap2);
  auto shot = [&]() {
    fill_u64(ctx, (u64 *)ctr, nctr, 0);
    if (ctx->time_kernels) HIP_CHECK(hipEventRecord(ctx->ev_a, ctx->stream));
    launch(pq.q);
    if (ctx->time_kernels) HIP_CHECK(hipEventRecord(ctx->ev_b, ctx->stream));
  };
  shot();
  unsigned long long *MB =
      (unsigned long long *)d2h_pinned(ctx, ctr, 8 * nctr);
  ProbeCounts r{MB[0], MB[1], nctr > 2 ? MB[2] : 0};
  u64 launches = 1;
  if (r.M > cap || r.E > cap2) {  // rare: queue overflow — exact relaunch
    pq.free(ctx);
    pq.alloc(ctx, std::max<u64>(r.M, 1), std::max<u64>(r.E, 1));
    shot();
    launches = 2;
  }
  if (ctx->time_kernels) {
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b));
    ctx->probe_ms += ms;
    ctx->probe_rows += n;
    ctx->probe_launches += launches;
    ctx->probe_pairs += r.M;
  }
  return r;
}

// Error stream of a finished probe: consolidate the E raw rows by
// (code, time) — the err collection is a first-class update stream in
// the reference (linear_join.rs:516-541) — free the raw columns, attach.
static void attach_err_stream(Ctx *ctx, mz_gpu_out *out, ProbeQueue &pq,
                              u64 E) {
  FlatCols ce;
  u64 Ec = 0;
  if (E) {
    DevUpdates epin{pq.q.ecodes, nullptr, pq.q.etimes, pq.q.ediffs, E};
    ce = consolidate_dev(ctx, 1, 0, epin, &Ec);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    dfree(ctx, ce.vals);  // codes are the key column; no vals
  }
  pq.free_errs(ctx);
  out_attach_errs(out, ce.keys, ce.times, ce.diffs, Ec);
}

// varlen probe host path (halfjoin / linear join over a varlen lookup):
// validates the closure shape, runs k_probe_vl with row+byte queues,
// consolidates (canonical varlen order) and returns a varlen out-batch.
static int probe_vl_impl(Ctx *ctx, mz_gpu_arr *lookup,
                         const mz_gpu_updates *u, u32 stream_vb, int mode,
                         int swap, const mz_gpu_closure *cl,
                         mz_gpu_out **out) {
  probe_prepare(ctx, lookup, mode, u->upper);
  u32 kw = lookup->schema.kw;
  u32 okw = cl->out.key_words;
  // closure validation: no reference to the varlen side except the
  // single whole-val passthrough
  u8 banned = swap ? MZ_SRC_VAL_STREAM : MZ_SRC_VAL_LOOKUP;
  for (u32 i = 0; i < cl->n_filters; i++)
    if (cl->filters[i].src == banned ||
        cl->filters[i].src == MZ_SRC_COMPUTE) {
      ctx->err = "varlen probe: filters may not touch the varlen side";
      return -1;
    }
  for (u32 i = 0; i < cl->n_key_fields; i++)
    if (cl->key_fields[i].src == banned) {
      ctx->err = "varlen probe: key fields may not touch the varlen side";
      return -1;
    }
  if (!(cl->n_val_fields == 1 && cl->val_fields[0].src == banned &&
        cl->val_fields[0].width == 0) ||
      cl->out.val_bytes != 0xFFFFFFFFu) {
    ctx->err = "varlen probe: out val must be the whole varlen val "
               "(one field, src = lookup side, width 0)";
    return -1;
  }
  mz_gpu_closure cl2 = *cl;
  cl2.n_val_fields = 0;  // key fields evaluated in-kernel; val is copied
  BatchList bl;
  build_probe_batchlist(ctx, lookup, u->lower, bl);
  (*ctx->scr).reset();
  DevUpdates d = stage_updates(ctx, u, kw, stream_vb);
  u64 n = d.n;
  if (n == 0 || bl.n == 0) {
    *out = empty_out_vl(ctx, okw);
    return 0;
  }
  u64 cap = 2 * n + 1024;
  DeltaView dv{d.keys, d.vals, stream_vb, d.times, d.diffs, n, kw};
  VlProbeQueue pq{okw};
  ProbeCounts r = run_probe(ctx, pq, cap, 64 * cap, 2, n, [&](VlQueue q) {
    hipLaunchKernelGGL(k_probe_vl, dim3(ngrid(n * (u64)bl.n)), dim3(BLK), 0,
                       ctx->stream, dv, bl, mode, swap, cl2, q);
  });
  VlCols cc = consolidate_vl(ctx, okw, pq.q.okeys, pq.q.ovstarts,
                             pq.q.ovends, pq.q.oarena, pq.q.otimes,
                             pq.q.odiffs, r.M);
  pq.free(ctx);
  *out = make_out_vl(cc.keys, cc.arena, cc.voffs, cc.times, cc.diffs, cc.n,
                     cc.bytes, okw);
  return 0;
}

struct mz_gpu_ctx {
  Ctx impl;
};

static void arr_flush_impl(Ctx *ctx, mz_gpu_arr *a);
// frees a collation's stitch state and minmax parts (its accumulable
// sub-reduce lives in ctx->reds); defined with the operator
static void collation_free(mz_gpu_ctx *c, mz_gpu_collation *op);
// frees a temporal filter's held buffer; defined with the operator
static void temporal_free(Ctx *ctx, struct mz_gpu_temporal *op);

// The reduce operator's device state: accumulator table, counters and the
// distinct aggregates' pair tables.
static void red_free_state(Ctx *ctx, mz_gpu_red *r) {
  kt_free(ctx, r->tbl);
  for (u32 j = 0; j < r->n_dist; j++) kt_free(ctx, r->ptbl[j]);
  dfree(ctx, r->d_ctr);
}

// Create-time rules for a distinct aggregate (mz_gpu.h); nullptr = ok.
static const char *distinct_agg_error(const mz_gpu_aggregate &g,
                                      const mz_gpu_schema &in) {
  if (!agg_is_distinct(g)) return nullptr;
  if (g.func == MZ_AGG_SUM_F64 || g.is_float)
    return "DISTINCT over a float datum is unsupported (float Datum "
           "equality is not byte equality)";
  if (g.width != 4 && g.width != 8)
    return "DISTINCT datum width must be 4 or 8";
  if ((u64)g.off + g.width + (g.nullable ? 1 : 0) > in.val_bytes)
    return "DISTINCT datum reads past in.val_bytes";
  return nullptr;
}

// ---- snapshot-diff push protocol: the operators that keep
// their groups' contents in an arrangement of their own (TopK, window
// functions) and answer a push with f(new snapshot) - f(old snapshot) of
// the changed groups.

static int probe_impl(Ctx *ctx, mz_gpu_arr *lookup, const mz_gpu_updates *u,
                      u32 stream_vb, int mode, int swap,
                      const mz_gpu_closure *cl, int consolidate_out,
                      mz_gpu_out **out);
static DevBatch *arr_insert_dev(Ctx *ctx, mz_gpu_arr *a, DevUpdates d,
                                u64 lower, u64 upper);

// Pass-through closure: the probe reads each (key, val, net) of the probed
// keys unchanged (the peek shape).
static void pass_through_closure(u32 kw, u32 vb, mz_gpu_closure &cl) {
  std::memset(&cl, 0, sizeof(cl));
  cl.n_key_fields = 1;
  cl.key_fields[0] = mz_gpu_field{MZ_SRC_KEY, 0, (u8)(8 * kw), 0, 0, 0, 0};
  cl.n_val_fields = vb ? 1u : 0u;
  if (vb)
    cl.val_fields[0] =
        mz_gpu_field{MZ_SRC_VAL_LOOKUP, 0, (u8)vb, 0, 0, 0, 0};
  cl.out.key_words = kw;
  cl.out.val_bytes = vb;
}

// One slice's correction rows: n rows in columns the operator allocated
// with flat_alloc and the driver frees.
struct SnapSeg {
  FlatCols cols;
  u64 n = 0;
};

// The push. The operator supplies
//   eval(t, oldp, newp, &seg) -> bool: evaluate the two consolidated
//     snapshots of one slice's changed groups (either may have no rows) into
//     seg, old rows with sign -1 and new rows with +1, all at time t. Scratch
//     is free for it. false stops the push; errors() must then say why.
//   errors(total) -> nullptr or the message: called once, after everything
//     queued has been synchronised, with the number of correction rows;
//     total > max_rows was not consolidated and must be refused here.
// A failed push leaves *out untouched and the slices installed so far
// installed.
template <class Eval, class Errors>
static int snapshot_diff_push(mz_gpu_ctx *c, mz_gpu_arr *arr, u32 out_vb,
                              u64 max_rows, const mz_gpu_updates *u,
                              Eval &&eval, Errors &&errors,
                              mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  const u32 kw = arr->schema.kw, vb = arr->schema.vb;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  u64 n = d.n;
  if (n == 0) {
    *out = empty_out(ctx, kw, out_vb);
    return 0;
  }
  // Owned sorted columns: they outlive spine merges' scratch resets.
  FlatCols s = flat_alloc(ctx, n, kw, vb);
  sort_gather(ctx, d.keys, kw, d.vals, vb, d.times, d.diffs, n, &s);
  mz_gpu_closure cl;
  pass_through_closure(kw, vb, cl);
  std::vector<SnapSeg> segs;
  u64 total = 0;
  int rc = 0;
  bool stopped = false;
  for (auto [lo, hi, t] : time_slices(ctx, s.times, n, u->lower, u->upper)) {
    u64 m = hi - lo;
    Groups g = group_sorted(ctx, s.keys + lo * kw, kw, s.times + lo, m);
    u64 G = *(u32 *)d2h_pinned(ctx, g.gid + (m - 1), 4);
    // the probe delta: one row per changed group at time t
    u64 *dg = dnew<u64>(ctx, G * kw);
    u64 *gt = dnew<u64>(ctx, G);
    i64 *gd = dnew<i64>(ctx, G);
    hipLaunchKernelGGL(k_gather_group_keys, dim3(ngrid(G)), dim3(BLK), 0,
                       ctx->stream, s.keys + lo * kw, kw, g.starts, g.gid, m,
                       dg);
    fill_u64(ctx, gt, G, t);
    fill_u64(ctx, (u64 *)gd, G, 1);
    mz_gpu_updates su{};
    su.keys = dg;
    su.vals = nullptr;
    su.times = gt;
    su.diffs = gd;
    su.n = G;
    su.lower = t;
    su.upper = t + 1;
    su.on_device = 1;
    // snapshot the changed groups, install the slice, snapshot again
    mz_gpu_out *oldp = nullptr, *newp = nullptr;
    rc = probe_impl(ctx, arr, &su, 0, PM_HALF_LE, 0, &cl, 1, &oldp);
    if (!rc) {
      DevUpdates sl{s.keys + lo * kw, s.vals + lo * vb, s.times + lo,
                    s.diffs + lo, m};
      arr_insert_dev(ctx, arr, sl, t, t + 1);
      rc = probe_impl(ctx, arr, &su, 0, PM_HALF_LE, 0, &cl, 1, &newp);
    }
    if (!rc) {
      SnapSeg seg;
      stopped = !eval(t, oldp, newp, &seg);
      if (seg.cols.keys) {
        segs.push_back(seg);
        total += seg.n;
      }
    }
    if (oldp) mz_gpu_out_release(c, oldp);
    if (newp) mz_gpu_out_release(c, newp);
    dfree(ctx, dg);
    dfree(ctx, gt);
    dfree(ctx, gd);
    if (rc || stopped) break;
  }
  const char *why = nullptr;
  if (!rc) {
    // one slice (the steady state) is consolidated where it was emitted
    const bool emitted = !stopped && total && total <= max_rows;
    FlatCols all, o;
    u64 Mc = 0;
    if (emitted) {
      all = segs[0].cols;
      if (segs.size() > 1) {
        all = flat_alloc(ctx, total, kw, out_vb);
        u64 base = 0;
        for (const SnapSeg &sg : segs) {
          HIP_CHECK(hipMemcpyAsync(all.keys + base * kw, sg.cols.keys,
                                   sg.n * kw * 8, hipMemcpyDeviceToDevice,
                                   ctx->stream));
          if (out_vb)
            HIP_CHECK(hipMemcpyAsync(all.vals + base * out_vb, sg.cols.vals,
                                     sg.n * out_vb, hipMemcpyDeviceToDevice,
                                     ctx->stream));
          HIP_CHECK(hipMemcpyAsync(all.times + base, sg.cols.times, sg.n * 8,
                                   hipMemcpyDeviceToDevice, ctx->stream));
          HIP_CHECK(hipMemcpyAsync(all.diffs + base, sg.cols.diffs, sg.n * 8,
                                   hipMemcpyDeviceToDevice, ctx->stream));
          base += sg.n;
        }
      }
      DevUpdates pin{all.keys, all.vals, all.times, all.diffs, total};
      o = consolidate_dev(ctx, kw, out_vb, pin, &Mc);
    }
    why = errors(total);
    if (emitted && segs.size() > 1) flat_free(ctx, all);
    if (why)
      flat_free(ctx, o);
    else
      *out = emitted ? make_out(o, Mc, kw, out_vb)
                     : empty_out(ctx, kw, out_vb);
  }
  for (SnapSeg &sg : segs) flat_free(ctx, sg.cols);
  flat_free(ctx, s);
  if (rc) return rc;
  if (why) {
    ctx->err = why;
    return -1;
  }
  return 0;
}

extern "C" {

mz_gpu_ctx *mz_gpu_init(const mz_gpu_cfg *cfg) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return nullptr;
  int dev = cfg ? (int)cfg->device_index : 0;
  HIP_CHECK(hipSetDevice(dev));
  mz_gpu_ctx *c = new mz_gpu_ctx();
  HIP_CHECK(hipStreamCreate(&c->impl.stream));
  c->impl.main_stream = c->impl.stream;
  c->impl.scr = &c->impl.scratch;
  HIP_CHECK(hipEventCreate(&c->impl.ev_a));
  HIP_CHECK(hipEventCreate(&c->impl.ev_b));
  HIP_CHECK(hipHostMalloc(&c->impl.pin, 4096));
  // Keep freed stream-ordered allocations in the pool forever (288 GB of
  // HBM — never hand memory back to the OS mid-run; pool misses showed up
  // as multi-ms host stalls before large allocations).
  hipMemPool_t pool = nullptr;
  if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool) {
    uint64_t thresh = UINT64_MAX;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold,
                                 &thresh);
  }
  // pre-grow the scratch arena so per-call growth never stalls the step
  u64 scratch0 = cfg && cfg->hbm_pool_bytes ? cfg->hbm_pool_bytes
                                            : (4ull << 30);
  void *warm = (*c->impl.scr).get(scratch0);
  // touch the arena once: un-backed pages otherwise fault in lazily
  // across the first process's timed steps (measured ~2x first-process
  // slowdown on some pool boxes)
  (void)hipMemsetAsync(warm, 0, scratch0, c->impl.stream);
  (*c->impl.scr).reset();
  // pre-back the async mempool the same way (spine batches and merge
  // outputs allocate from it at 32MB size classes)
  {
    // allocate all, touch all, then free all — alloc/free pairs would
    // recycle one block and back only 2GB
    void *ps[12] = {};
    for (int i = 0; i < 12; i++) {
      if (hipMallocAsync(&ps[i], 2ull << 30, c->impl.stream) !=
          hipSuccess)
        ps[i] = nullptr;
      if (ps[i])
        (void)hipMemsetAsync(ps[i], 0, 2ull << 30, c->impl.stream);
    }
    for (int i = 0; i < 12; i++)
      if (ps[i]) (void)hipFreeAsync(ps[i], c->impl.stream);
  }
  (void)hipStreamSynchronize(c->impl.stream);
  const char *prof = getenv("MZ_GPU_PROF");
  c->impl.prof.enabled = prof && prof[0] && prof[0] != '0';
  return c;
}

// Sub-phase profile dump (MZ_GPU_PROF=1): per category, total device ms
// over the recorded event pairs since the last dump. Printed to stderr as
// "MZPROF <cat> <ms> <count>" lines; events are released. Event pairs may
// live on per-arrangement lane streams, so all lanes are synced first.
void mz_gpu_prof_dump(mz_gpu_ctx *c) {
  Ctx *ctx = &c->impl;
  if (!ctx->prof.enabled) return;
  for (mz_gpu_arr *a : ctx->arrs)
    if (a->stream) (void)hipStreamSynchronize(a->stream);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &[name, evs] : ctx->prof.cats) {
    double total = 0;
    for (auto &[a, b] : evs) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, a, b) == hipSuccess) total += ms;
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
    fprintf(stderr, "MZPROF %s %.3f %zu\n", name.c_str(), total,
            evs.size());
  }
  fflush(stderr);
  ctx->prof.cats.clear();
}

// Arrangement teardown, shared by mz_gpu_arr_drop and mz_gpu_fini. First
// the lane and merge-stream resources (each stream is drained before it is
// destroyed), then the device state, freed on the ctx stream.
static void arr_release_lanes(mz_gpu_arr *a) {
  if (a->stream) {
    (void)hipStreamSynchronize(a->stream);
    (void)hipStreamDestroy(a->stream);
    (void)hipEventDestroy(a->ev_done);
    (void)hipEventDestroy(a->ev_gate);
    (void)hipEventDestroy(a->ev_ready);
    if (a->lane_scr) a->lane_scr->destroy();
    delete a->lane_scr;
    a->stream = nullptr;
    a->lane_scr = nullptr;
  }
  if (a->mstream) {
    (void)hipStreamSynchronize(a->mstream);
    (void)hipStreamDestroy(a->mstream);
    (void)hipEventDestroy(a->ev_mdone);
    if (a->merge_scr) a->merge_scr->destroy();
    delete a->merge_scr;
    a->mstream = nullptr;
    a->merge_scr = nullptr;
  }
}

static void arr_release_state(Ctx *ctx, mz_gpu_arr *a) {
  for (auto &b : a->batches) free_batch(ctx, b);
  a->batches.clear();
  flat_free(ctx, a->pending.flat);
  dfree(ctx, a->sort_plan.dev);
  dfree(ctx, a->sort_plan.d_flag);
  if (a->pending.active) free_batch(ctx, a->pending.batch);
  if (a->pending_merge.active) free_batch(ctx, a->pending_merge.merged);
}

void mz_gpu_fini(mz_gpu_ctx *c) {
  if (!c) return;
  Ctx *ctx = &c->impl;
  // release everything the library owns: lane resources, arrangement
  // batches, operator state tables, scratch arenas (leaking these across
  // many short-lived contexts exhausted HBM)
  for (mz_gpu_arr *a : ctx->arrs) arr_release_lanes(a);
  (void)hipStreamSynchronize(ctx->stream);
  const char *dbg = getenv("MZ_DBG_FINI");
  for (mz_gpu_arr *a : ctx->arrs) {
    if (dbg) fprintf(stderr, "[fini] arr %p batches=%zu\n", (void *)a,
                     a->batches.size());
    arr_release_state(ctx, a);
    delete a;
  }
  ctx->arrs.clear();
  for (mz_gpu_red *r : ctx->reds) {
    if (dbg) fprintf(stderr, "[fini] red %p\n", (void *)r);
    red_free_state(ctx, r);
    delete r;
  }
  ctx->reds.clear();
  for (mz_gpu_collation *co : ctx->cols) collation_free(c, co);
  ctx->cols.clear();
  for (mz_gpu_temporal *tf : ctx->temporals) temporal_free(ctx, tf);
  ctx->temporals.clear();
  for (mz_gpu_join *j : ctx->joins) delete j;
  ctx->joins.clear();
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->pin) (void)hipHostFree(ctx->pin);
  ctx->scratch.destroy();
  // hand the pool's now-unused reservations back to the OS: the infinite
  // release threshold (set in init for steady-state speed) otherwise
  // accumulates reserved-but-free memory across short-lived contexts
  // until plain hipMalloc (scratch arenas) cannot back a new one
  if (!getenv("MZ_NO_TRIM")) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool)
      (void)hipMemPoolTrimTo(pool, 0);
  }
  delete c;
}

const char *mz_gpu_last_error(mz_gpu_ctx *c) { return c->impl.err.c_str(); }

int mz_gpu_sync(mz_gpu_ctx *c) {
  for (mz_gpu_arr *a : c->impl.arrs) {
    arr_flush_impl(&c->impl, a);
    merge_finish(&c->impl, a);
    if (a->stream) HIP_CHECK(hipStreamSynchronize(a->stream));
    if (a->mstream) HIP_CHECK(hipStreamSynchronize(a->mstream));
  }
  HIP_CHECK(hipStreamSynchronize(c->impl.stream));
  return 0;
}

mz_gpu_arr *mz_gpu_arr_create(mz_gpu_ctx *c, const mz_gpu_schema *s) {
  mz_gpu_arr *a = new mz_gpu_arr();
  a->schema = {s->key_words, s->val_bytes};
  c->impl.arrs.push_back(a);
  return a;
}

void mz_gpu_arr_drop(mz_gpu_ctx *c, mz_gpu_arr *a) {
  Ctx *ctx = &c->impl;
  arr_flush_impl(ctx, a);
  merge_finish(ctx, a);  // an in-flight deferred merge reads the batches
  // full teardown: lane resources, device state, registry entry, the
  // struct itself
  arr_release_lanes(a);
  arr_release_state(ctx, a);
  auto &v = ctx->arrs;
  v.erase(std::remove(v.begin(), v.end(), a), v.end());
  delete a;
}

// Geometric spine maintenance (amortized merging — scheduling policy per
// DESIGN.md §2.4; semantics = DD Spine merges with logical compaction):
// keep batch sizes decreasing by >=2x tail-to-head; merging the tail
// whenever the invariant breaks costs O(log) amortized merge work per
// update and keeps the probe fan-out at ~log(arrangement/batch).
//
// The knobs, read once per process at the first policy decision.
// Large batches keep the geometric pair rule (merge-path pair merges
// are O(n)); small batches pool lazily and merge k-way when the pool
// exceeds its depth — per-merge fixed overhead (~25 kernel launches +
// syncs) made per-step pair merges of 100k-row batches the dominant step
// cost.
struct SpineKnobs {
  // MZ_GPU_SMALL, 4M default: measured 2x on the 1M-row churn config
  // (per-step pair merges of 1M batches into the resident run were the
  // dominant cost; pooling amortizes the big merge over POOL steps).
  // 4M/6 defaults: measured best at honest steady state (20-step runs
  // spanning full pool cycles: 4.06 ms/step vs 12.6 at 8M/8 — deep pools
  // inflate probe fan-out and the amortized big-run rewrite; per-step
  // pair merges without pooling ran 10+ ms/step).
  u64 small;
  // MZ_GPU_SMALL_POOL pins a fixed pool depth; -1 = adaptive on batch
  // size (A/B-measured on the final build): probing costs ~64 B/delta-row
  // per pooled batch, merging costs one k-way rewrite per cycle. Small
  // per-step batches amortize merges best with a DEEP pool (100k rows:
  // pool 8 beat 6 by 6%); large batches pay more for probe fan-out than
  // merges, so a SHALLOW pool wins (1M rows: pool 4 beat 6 by 22%).
  long pool;
  // MZ_GPU_GEO=1.0: merge the run below only once the new run matches its
  // size (tiering-leaning). The leveling factor 2.0 re-rewrote the big
  // resident run on a cascade every ~30 steps: 109+184ms giant-merge
  // steps vs 51ms at 1.0 (12.1 -> 5.6 ms/step avg over 36-step windows).
  double geo;
};
static const SpineKnobs &spine_knobs() {
  static const SpineKnobs K = [] {
    const char *s = getenv("MZ_GPU_SMALL");
    const char *p = getenv("MZ_GPU_SMALL_POOL");
    const char *g = getenv("MZ_GPU_GEO");
    return SpineKnobs{s ? (u64)atoll(s) : (u64)(4u << 20), p ? atol(p) : -1,
                      g ? atof(g) : 1.0};
  }();
  return K;
}

// One policy decision over the batch sizes: the range [from, to) the given
// rule wants merged now, or from == to for none.
enum SpineRule { RULE_PAIR, RULE_POOL, RULE_CAP };
struct MergeDue {
  size_t from = 0, to = 0;
  explicit operator bool() const { return to > from; }
};
static MergeDue spine_due(const mz_gpu_arr *a, SpineRule rule) {
  const SpineKnobs &K = spine_knobs();
  const auto &B = a->batches;
  size_t nb = B.size();
  switch (rule) {
    case RULE_PAIR:  // the last run has caught up with the one below it
      if (nb >= 2 &&
          (double)B[nb - 2].n_upds <= K.geo * (double)B[nb - 1].n_upds &&
          B[nb - 2].n_upds + B[nb - 1].n_upds >= K.small)
        return {nb - 2, nb};
      break;
    case RULE_POOL: {  // the trailing small batches outgrew the pool
      size_t i = nb;
      while (i > 0 && B[i - 1].n_upds < K.small) i--;
      long depth = K.pool;
      if (depth < 0) {
        u64 last = B.empty() ? 0 : B.back().n_upds;
        depth = last >= (512u << 10) ? 4 : last <= (256u << 10) ? 8 : 6;
      }
      if ((long)(nb - i) > depth) return {i, nb};
      break;
    }
    case RULE_CAP:  // hard cap: the probe BatchList's capacity
      if (nb > 10) return {0, nb};
      break;
  }
  return {};
}

// Synchronous driver: the pair rule until it rests, the pool rule once,
// then the cap.
static void spine_policy(Ctx *ctx, mz_gpu_arr *a) {
  while (MergeDue m = spine_due(a, RULE_PAIR))
    merge_range(ctx, a, m.from, m.to);
  if (MergeDue m = spine_due(a, RULE_POOL)) merge_range(ctx, a, m.from, m.to);
  while (MergeDue m = spine_due(a, RULE_CAP))
    merge_range(ctx, a, m.from, m.to);
}

// Deferred driver: enqueue at most ONE merge (the innermost due) per call
// on the merge stream; cascades progress one merge per flush, off the
// probe critical path. The hard cap stays synchronous.
static void spine_policy_deferred(Ctx *ctx, mz_gpu_arr *a) {
  if (a->pending_merge.active) return;  // one in flight per arrangement
  for (SpineRule rule : {RULE_PAIR, RULE_POOL})
    if (MergeDue m = spine_due(a, rule)) {
      MergeGuard mg(ctx, a);
      merge_range(ctx, a, m.from, m.to, 1);
      return;
    }
  while (MergeDue m = spine_due(a, RULE_CAP))
    merge_range(ctx, a, m.from, m.to);
}

int mz_gpu_arr_push_batch(mz_gpu_ctx *c, mz_gpu_arr *a,
                          const mz_gpu_updates *u) {
  Ctx *ctx = &c->impl;
  if (is_varlen(a->schema.vb)) {
    arr_insert_vl(ctx, a, u);  // sealed input re-consolidates (idempotent)
    return 0;
  }
  arr_flush_impl(ctx, a);
  LaneGuard lane(ctx, a);
  (*ctx->scr).reset();
  u32 kw = a->schema.kw, vb = a->schema.vb;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  // copy into owned arrays (batch owns its storage)
  FlatCols f = flat_alloc(ctx, d.n, kw, vb);
  if (d.n) {
    HIP_CHECK(hipMemcpyAsync(f.keys, d.keys, d.n * kw * 8,
                             hipMemcpyDeviceToDevice, ctx->stream));
    if (vb)
      HIP_CHECK(hipMemcpyAsync(f.vals, d.vals, d.n * vb,
                               hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(f.times, d.times, d.n * 8,
                             hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(f.diffs, d.diffs, d.n * 8,
                             hipMemcpyDeviceToDevice, ctx->stream));
  }
  DevBatch b = build_batch(ctx, kw, vb, f.keys, f.vals, f.times, f.diffs,
                           d.n, u->lower, u->upper);
  a->batches.push_back(b);
  a->upper = std::max(a->upper, u->upper);
  spine_policy(ctx, a);
  (void)hipEventRecord(a->ev_ready, ctx->stream);
  return 0;
}

// Seal + install + policy over already-staged device updates, on the
// current lane, with one sync (the counts read); returns a pointer to the
// pushed batch (valid until the next spine merge).
static DevBatch *arr_insert_dev(Ctx *ctx, mz_gpu_arr *a, DevUpdates d,
                                u64 lower, u64 upper) {
  MZ_PROF(ctx, "arr_insert");
  Sealed s = seal_updates(ctx, a->schema.kw, a->schema.vb, d, lower, upper,
                          nullptr, 0);
  set_counts(s.batch, (u64 *)d2h_pinned(ctx, s.dcounts, 3 * 8));
  a->batches.push_back(s.batch);
  a->upper = std::max(a->upper, upper);
  spine_policy(ctx, a);
  return &a->batches.back();
}

// varlen insert: synchronous consolidate + build + push (no lane
// pipeline — varlen is off the benchmark hot path)
static void arr_insert_vl(Ctx *ctx, mz_gpu_arr *a,
                          const mz_gpu_updates *u) {
  (*ctx->scr).reset();
  u32 kw = a->schema.kw;
  DevUpdates d = stage_updates(ctx, u, kw, a->schema.vb);
  // copy-consolidate then seal: consolidate_vl owns fresh arrays
  VlCols cc = consolidate_vl(ctx, kw, d.keys,
                             d.val_offs, d.val_offs + 1, d.vals, d.times,
                             d.diffs, d.n);
  DevBatch b = build_batch_vl(ctx, kw, std::move(cc), u->lower, u->upper);
  a->batches.push_back(b);
  a->upper = std::max(a->upper, u->upper);
  spine_policy(ctx, a);
  if (a->stream) (void)hipEventRecord(a->ev_ready, a->stream);
}

// Enqueue-only half of an insert: the seal runs on the arrangement's own
// lane; the counts readback is issued asynchronously and the sealed batch
// joins the spine at mz_gpu_arr_flush. Independent arrangements' inserts
// overlap this way (one per GPU stream). `plan` non-null (device inputs only)
// uses the arrangement's cached sort plan without the minmax sync; the
// device validity flag is copied back with the counts and checked at
// the flush, which rebuilds synchronously on a mismatch (rare: the
// batch's column ranges escaped the cached bounds).
static void insert_pipeline(Ctx *ctx, mz_gpu_arr *a, DevUpdates d,
                            u64 lower, u64 upper,
                            mz_gpu_arr::SortPlan *plan) {
  // NOTE: does NOT reset the lane scratch — host-input callers staged
  // `d` into it (arr_insert_async_impl resets before staging)
  if (plan && plan->d_flag) fill_u32(ctx, plan->d_flag, 1, 0);
  Sealed s = seal_updates(ctx, a->schema.kw, a->schema.vb, d, lower, upper,
                          plan, /*keep_flat=*/1);
  a->pending.active = 1;
  a->pending.batch = s.batch;
  a->pending.staged = d;
  a->pending.lower = lower;
  a->pending.upper = upper;
  a->pending.flat = s.flat;
  a->pending.flag[0] = 0;
  HIP_CHECK(hipMemcpyAsync(a->pending.cnt, s.dcounts, 3 * 8,
                           hipMemcpyDeviceToHost, ctx->stream));
  if (plan && plan->d_flag)
    HIP_CHECK(hipMemcpyAsync(a->pending.flag, plan->d_flag, 4,
                             hipMemcpyDeviceToHost, ctx->stream));
}

static void arr_insert_async_impl(Ctx *ctx, mz_gpu_arr *a,
                                  const mz_gpu_updates *u) {
  MZ_PROF(ctx, "arr_insert");
  if (is_varlen(a->schema.vb)) {
    arr_insert_vl(ctx, a, u);
    return;
  }
  if (a->pending.active) arr_flush_impl(ctx, a);
  // gate=false: this pipeline writes only freshly-allocated memory, so
  // it may run concurrently with the main stream's in-flight probes of
  // the arrangement's CURRENT batches (the 1-deep insert pipeline).
  LaneGuard lane(ctx, a, /*gate=*/false);
  (*ctx->scr).reset();
  DevUpdates d = stage_updates(ctx, u, a->schema.kw, a->schema.vb);
  // the cached-plan path needs the inputs retained for the redo; only
  // device inputs outlive the call (the async-insert lifetime contract)
  static const bool NO_PLAN_CACHE = [] {
    const char *e = getenv("MZ_NO_SORT_PLAN_CACHE");
    return e && e[0] && e[0] != '0';
  }();
  mz_gpu_arr::SortPlan *plan =
      (!NO_PLAN_CACHE && u->on_device && !d.sorted) ? &a->sort_plan
                                                    : nullptr;
  insert_pipeline(ctx, a, d, u->lower, u->upper, plan);
}

static void arr_flush_take_impl(Ctx *ctx, mz_gpu_arr *a,
                                mz_gpu_out **take) {
  if (take) *take = nullptr;
  if (!a->pending.active && !a->pending_merge.active) return;
  MZ_PROF(ctx, "arr_flush");
  // gate=false: the flush waits only for the LANE's own pipeline (the
  // pending consolidation/merge), not for the main stream's in-flight
  // probes of the previous step — installs mutate only the host batch
  // list, and retired batches are freed on the main stream (free_batch),
  // in-order after every probe that reads them.
  LaneGuard lane(ctx, a, /*gate=*/false);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (a->pending.active && a->pending.flag[0]) {
    // the cached sort plan did not cover this batch: discard the
    // mis-sorted build and redo synchronously (re-priming the cache)
    free_batch(ctx, a->pending.batch);
    flat_free(ctx, a->pending.flat);
    a->sort_plan.valid = 0;
    (*ctx->scr).reset();  // redo inputs are device-resident, not staged
    insert_pipeline(ctx, a, a->pending.staged, a->pending.lower,
                    a->pending.upper, &a->sort_plan);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  // install an in-flight deferred merge only when its stream is done —
  // otherwise leave it running (the pre-merge batch list stays valid)
  if (a->pending_merge.active &&
      (!a->ev_mdone || hipEventQuery(a->ev_mdone) == hipSuccess))
    merge_install(ctx, a);
  if (a->pending.active) {
    DevBatch b = a->pending.batch;
    set_counts(b, a->pending.cnt);
    a->batches.push_back(b);
    a->upper = std::max(a->upper, a->pending.upper);
    a->pending.active = 0;
    u32 kw = a->schema.kw, vb = a->schema.vb;
    if (take && b.n_upds) {
      // hand the consolidated flat rows over as a sorted out-batch that
      // owns its four columns (the batch owns its own times/diffs, which
      // a spine merge may free). The lane wrote them all before the
      // synchronisation above, so the out's consumers, which run on
      // other streams, find them complete.
      *take = make_out(a->pending.flat, b.n_upds, kw, vb);
      a->pending.flat = FlatCols();
    } else {
      flat_free(ctx, a->pending.flat);
    }
  }
  // Synchronous merges by default: deferral was re-measured (round 2)
  // with the merge on its OWN stream + own scratch + event-gated
  // install, and still loses on BOTH configs (100k: 2.50 vs 2.26
  // ms/step; 1M: 9.3 vs 5.9) — probes pay ~64 B/row for every extra
  // batch in the pre-merge list (the fused two-stage probe doubly so),
  // and at 1M the merges are bandwidth-bound, so the overlap has no
  // spare bandwidth to use. MZ_GPU_DEFER_MERGE=1 enables the
  // merge-stream deferral for latency-sensitive shapes. ev_ready (what
  // probes wait on) is recorded BEFORE a deferred merge but AFTER
  // synchronous ones.
  static const bool DEFER = [] {
    const char *e = getenv("MZ_GPU_DEFER_MERGE");
    return e && e[0] && e[0] != '0';
  }();
  if (DEFER) {
    (void)hipEventRecord(a->ev_ready, ctx->stream);
    spine_policy_deferred(ctx, a);
  } else {
    spine_policy(ctx, a);
    (void)hipEventRecord(a->ev_ready, ctx->stream);
  }
}

static void arr_flush_impl(Ctx *ctx, mz_gpu_arr *a) {
  arr_flush_take_impl(ctx, a, nullptr);
}

int mz_gpu_arr_insert_async(mz_gpu_ctx *c, mz_gpu_arr *a,
                            const mz_gpu_updates *u) {
  arr_insert_async_impl(&c->impl, a, u);
  return 0;
}

int mz_gpu_arr_flush(mz_gpu_ctx *c, mz_gpu_arr *a) {
  arr_flush_impl(&c->impl, a);
  return 0;
}

int mz_gpu_arr_flush_take(mz_gpu_ctx *c, mz_gpu_arr *a, mz_gpu_out **out) {
  arr_flush_take_impl(&c->impl, a, out);
  return 0;
}

int mz_gpu_arr_insert(mz_gpu_ctx *c, mz_gpu_arr *a,
                      const mz_gpu_updates *u) {
  arr_insert_async_impl(&c->impl, a, u);
  arr_flush_impl(&c->impl, a);
  return 0;
}

int mz_gpu_arr_set_logical_compaction(mz_gpu_ctx *c, mz_gpu_arr *a,
                                      uint64_t f) {
  a->logical_compaction = f;
  return 0;
}

int mz_gpu_arr_set_physical_compaction(mz_gpu_ctx *c, mz_gpu_arr *a,
                                       uint64_t f) {
  (void)c;
  a->physical_compaction = f;  // recorded; eager level merges subsume it
  return 0;
}

int mz_gpu_arr_maintain(mz_gpu_ctx *c, mz_gpu_arr *a, uint64_t fuel) {
  (void)fuel;
  Ctx *ctx = &c->impl;
  arr_flush_impl(ctx, a);  // pending insert joins; pending merge installs
  LaneGuard lane(ctx, a);
  merge_finish(ctx, a);  // the flush's policy may have enqueued one
  merge_range(ctx, a, 0, a->batches.size());
  return 0;
}

int mz_gpu_arr_stats(mz_gpu_ctx *c, mz_gpu_arr *a, uint64_t *n_batches,
                     uint64_t *n_updates, uint64_t *hbm_bytes) {
  arr_flush_impl(&c->impl, a);
  *n_batches = a->batches.size();
  u64 n = 0, by = 0;
  u32 kw = a->schema.kw, vb = a->schema.vb;
  for (auto &b : a->batches) {
    n += b.n_upds;
    by += b.n_keys * kw * 8 + b.n_vals * vb + b.n_upds * 16 +
          b.hash_slots * (kw + 1) * 8 + (b.n_keys + b.n_vals) * 4 +
          b.n_upds * 4 + b.n_vals * 4;
  }
  *n_updates = n;
  *hbm_bytes = by;
  return 0;
}

void mz_gpu_out_release(mz_gpu_ctx *c, mz_gpu_out *o) {
  OutOwned *oo = reinterpret_cast<OutOwned *>(o);
  for (void *p : {(void *)oo->keys, (void *)oo->vals, (void *)oo->times,
                  (void *)oo->diffs, (void *)o->err_codes,
                  (void *)o->err_times, (void *)o->err_diffs,
                  (void *)o->val_offs})
    dfree(&c->impl, p);
  delete oo;
}

/* VARLEN out-batches: copy the [n+1] val offsets to the host. */
int mz_gpu_out_voffs_to_host(mz_gpu_ctx *c, const mz_gpu_out *o,
                             uint32_t *offs) {
  Ctx *ctx = &c->impl;
  HIP_CHECK(hipMemcpyAsync(offs, o->val_offs, (o->n + 1) * 4,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mz_gpu_out_err_to_host(mz_gpu_ctx *c, const mz_gpu_out *o,
                           uint64_t *codes, uint64_t *times,
                           int64_t *diffs) {
  Ctx *ctx = &c->impl;
  u64 n = o->err_n;
  if (n == 0) return 0;
  HIP_CHECK(hipMemcpyAsync(codes, o->err_codes, n * 8,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(times, o->err_times, n * 8,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(diffs, o->err_diffs, n * 8,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mz_gpu_out_to_host(mz_gpu_ctx *c, const mz_gpu_out *o, uint64_t *keys,
                       uint8_t *vals, uint64_t *times, int64_t *diffs) {
  Ctx *ctx = &c->impl;
  u64 n = o->n;
  if (n == 0) return 0;
  u32 kw = o->schema.key_words, vb = o->schema.val_bytes;
  HIP_CHECK(hipMemcpyAsync(keys, o->keys, n * kw * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
  if (is_varlen(vb)) {
    if (o->val_arena_bytes)
      HIP_CHECK(hipMemcpyAsync(vals, o->vals, o->val_arena_bytes,
                               hipMemcpyDeviceToHost, ctx->stream));
  } else if (vb)
    HIP_CHECK(hipMemcpyAsync(vals, o->vals, n * vb, hipMemcpyDeviceToHost,
                             ctx->stream));
  HIP_CHECK(hipMemcpyAsync(times, o->times, n * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_CHECK(hipMemcpyAsync(diffs, o->diffs, n * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mz_gpu_consolidate(mz_gpu_ctx *c, const mz_gpu_schema *s,
                       const mz_gpu_updates *u, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  u32 kw = s->key_words, vb = s->val_bytes;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  if (is_varlen(vb)) {
    VlCols cc = consolidate_vl(ctx, kw, d.keys, d.val_offs,
                               d.val_offs + 1, d.vals, d.times, d.diffs,
                               d.n);
    *out = make_out_vl(cc.keys, cc.arena, cc.voffs, cc.times, cc.diffs,
                       cc.n, cc.bytes, kw);
    return 0;
  }
  u64 M;
  FlatCols o = consolidate_dev(ctx, kw, vb, d, &M);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = make_out(o, M, kw, vb);
  return 0;
}

mz_gpu_join *mz_gpu_join_create(mz_gpu_ctx *c, mz_gpu_arr *a1, mz_gpu_arr *a2,
                                const mz_gpu_closure *cl) {
  mz_gpu_join *j = new mz_gpu_join();
  j->arr1 = a1;
  j->arr2 = a2;
  j->cl = *cl;
  c->impl.joins.push_back(j);
  return j;
}

void mz_gpu_join_drop(mz_gpu_ctx *c, mz_gpu_join *j) {
  auto &v = c->impl.joins;
  v.erase(std::remove(v.begin(), v.end(), j), v.end());
  delete j;  // the operator does not own its input arrangements
}

// shared probe path for linear join and half join; consolidate_out=0
// skips the output consolidation (legal when the consumer consolidates —
// the reduce does — and an engine-internal optimization)
static int probe_impl(Ctx *ctx, mz_gpu_arr *lookup, const mz_gpu_updates *u,
                      u32 stream_vb, int mode, int swap,
                      const mz_gpu_closure *cl, int consolidate_out,
                      mz_gpu_out **out) {
  if (is_varlen(lookup->schema.vb))
    return probe_vl_impl(ctx, lookup, u, stream_vb, mode, swap, cl, out);
  probe_prepare(ctx, lookup, mode, u->upper);
  BatchList bl;
  build_probe_batchlist(ctx, lookup, u->lower, bl);
  (*ctx->scr).reset();
  auto &S = (*ctx->scr);
  u32 kw = lookup->schema.kw, lvb = lookup->schema.vb;
  u32 okw = cl->out.key_words, ovb = cl->out.val_bytes;
  DevUpdates d = stage_updates(ctx, u, kw, stream_vb);
  u64 n = d.n;
  if (n == 0 || bl.n == 0) {
    *out = empty_out(ctx, okw, ovb);
    return 0;
  }
  // SORTED deltas probe large batches by merge scan (k_probe_merge:
  // streaming both sorted sides); everything else takes the hash walk.
  // read per call (not latched): tests force the merge path with tiny
  // thresholds mid-process
  const char *emn = getenv("MZ_PROBE_MERGE_MIN_MB");
  const u64 MERGE_MIN = (u64)(emn ? atoll(emn) : 24) << 20;
  // Default OFF: measured 1.4x slower than the compressed-slot hash walk
  // at the Q3 1M config (LDS staging + lockstep searches beat by 16 B
  // random slots over half-L2-resident tables); kept as a parity-tested
  // option for larger-than-L2 regimes. MZ_PROBE_MERGE=1 enables.
  const char *eme = getenv("MZ_PROBE_MERGE");
  const bool MERGE_EN = eme && eme[0] == '1';
  BatchList blw;
  blw.n = 0;
  struct MergeTarget {
    DevBatch b;
    u8 allpass;
  };
  std::vector<MergeTarget> mts;
  for (int b2 = 0; b2 < bl.n; b2++) {
    u64 tb = bl.b[b2].hash_slots * (kw + 1) * 8;
    if (MERGE_EN && d.sorted && tb > MERGE_MIN && bl.b[b2].n_keys >= 4096)
      mts.push_back({bl.b[b2], bl.allpass[b2]});
    else {
      blw.b[blw.n] = bl.b[b2];
      blw.allpass[blw.n++] = bl.allpass[b2];
    }
  }
  u64 nb2 = n * (u64)blw.n;
  u64 mgrid = (n + MERGE_DROWS - 1) / MERGE_DROWS;
  u64 *mbounds = nullptr;
  if (!mts.empty()) {
    mbounds = (u64 *)S.get(mts.size() * mgrid * 2 * 8);
    for (size_t mi = 0; mi < mts.size(); mi++)
      hipLaunchKernelGGL(k_merge_bounds, dim3(ngrid(mgrid)), dim3(BLK), 0,
                         ctx->stream, d.keys, n, kw, mts[mi].b.keys,
                         mts[mi].b.n_keys, mgrid,
                         mbounds + mi * mgrid * 2);
  }
  // Queue sized from the arrangement's emit-ratio hint; error rows are
  // exceptional (exact relaunch).
  u64 cap = (lookup->probe_cap_hint ? lookup->probe_cap_hint + 1 : 2) * n +
            1024;
  DeltaView dv{d.keys, d.vals, stream_vb, d.times, d.diffs, n, kw};
  ProbeQueue pq{okw, ovb};
  ProbeCounts r =
      run_probe(ctx, pq, cap, n / 4 + 1024, 2, n, [&](EmitQueue q) {
        for (size_t mi = 0; mi < mts.size(); mi++)
          hipLaunchKernelGGL(k_probe_merge, dim3((u32)mgrid), dim3(BLK), 0,
                             ctx->stream, dv, lvb, mts[mi].b,
                             (int)mts[mi].allpass, mode, swap, *cl,
                             mbounds + mi * mgrid * 2, q);
        if (blw.n)
          hipLaunchKernelGGL(k_probe_walk, dim3(ngrid(nb2)), dim3(BLK), 0,
                             ctx->stream, dv, lvb, blw, mode, swap, *cl, q);
      });
  u64 M = r.M;
  lookup->probe_cap_hint = (M + n - 1) / n;
  if (ctx->time_kernels) {  // run_probe has synced and entered the call
    ctx->probe_batches += (u64)bl.n;
    // Algorithmic bytes of the probe (SURVEY §8d model, updated for the
    // compressed 16 B hash slots: one 64 B line per probed batch instead
    // of the r1 layout's 128 B): delta tuple + one hash line per batch +
    // matched val+upd read + output write — each touched once cold in
    // the single walk.
    ctx->probe_alg_bytes +=
        n * (8ull * kw + stream_vb + 16) + n * 64ull * (u64)bl.n +
        M * (lvb + 16ull) + M * (8ull * okw + ovb + 16);
  }
  if (!consolidate_out) {
    // raw emitted pairs (deterministic content; consumer consolidates)
    *out = make_out(pq.q.okeys, pq.q.ovals, pq.q.otimes, pq.q.odiffs, M,
                    okw, ovb);
  } else {
    DevUpdates pin{pq.q.okeys, pq.q.ovals, pq.q.otimes, pq.q.odiffs, M};
    u64 Mc;
    FlatCols o = consolidate_dev(ctx, okw, ovb, pin, &Mc);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    pq.free_ok(ctx);
    *out = make_out(o, Mc, okw, ovb);
  }
  attach_err_stream(ctx, *out, pq, r.E);
  return 0;
}

int mz_gpu_join_push(mz_gpu_ctx *c, mz_gpu_join *op, int side,
                     const mz_gpu_updates *delta, mz_gpu_out **out) {
  mz_gpu_arr *own = side == 1 ? op->arr1 : op->arr2;
  mz_gpu_arr *opp = side == 1 ? op->arr2 : op->arr1;
  // swap=1 when the delta is input 2 (closure args are (v1, v2) by input
  // number — mz_join_core.rs:69)
  return probe_impl(&c->impl, opp, delta, own->schema.vb, PM_JOIN,
                    side == 2 ? 1 : 0, &op->cl, 1, out);
}

int mz_gpu_halfjoin(mz_gpu_ctx *c, mz_gpu_arr *lookup,
                    const mz_gpu_updates *delta, uint32_t stream_val_bytes,
                    int le, const mz_gpu_closure *cl, mz_gpu_out **out) {
  return probe_impl(&c->impl, lookup, delta, stream_val_bytes,
                    le ? PM_HALF_LE : PM_HALF_LT, 0, cl, 1, out);
}

// Peek: read each requested key's (val, summed diff) as of `time` —
// a half-join (le) of the key list against the arrangement with the
// identity closure (handle_peek/process_peeks analog, compute_state.rs).
int mz_gpu_peek(mz_gpu_ctx *c, mz_gpu_arr *arr, const uint64_t *keys,
                uint64_t n_keys, uint64_t time, mz_gpu_out **out) {
  u32 kw = arr->schema.kw, vb = arr->schema.vb;
  std::vector<u64> times(n_keys, time);
  std::vector<i64> diffs(n_keys, 1);
  mz_gpu_updates u{};
  u.keys = keys;
  u.vals = nullptr;
  u.times = times.data();
  u.diffs = diffs.data();
  u.n = n_keys;
  u.lower = time;
  u.upper = time + 1;
  u.on_device = 0;
  mz_gpu_closure cl;
  pass_through_closure(kw, vb, cl);
  return probe_impl(&c->impl, arr, &u, 0, PM_HALF_LE, 0, &cl, 1, out);
}

// The closure shapes an MFP over one (key, val) row may take: the val is
// one of the closure's two val sides and the other, `absent`, does not
// exist (a full-scan peek has no stream side, a temporal filter no lookup
// side). Every read must stay inside the kw key words / vb val bytes.
// Returns the message, prefixed with `who`, or "" when the shape is fine.
static std::string mfp_shape_error(const char *who, const mz_gpu_closure *cl,
                                   u32 kw, u32 vb, u8 absent,
                                   const char *absent_why,
                                   const char *row_name) {
  const std::string w = std::string(who) + ": mfp ";
  if (cl->n_filters > MZ_GPU_MAX_FILTERS ||
      cl->n_key_fields > MZ_GPU_MAX_FIELDS ||
      cl->n_val_fields > MZ_GPU_MAX_FIELDS)
    return w + "filter/field count out of range";
  if (cl->out.key_words == 0 || cl->out.key_words > (u32)MAX_KW ||
      cl->out.val_bytes > (u32)MAX_VB)
    return w + "out schema unsupported (1..2 key words, "
               "fixed-width val of at most 64 bytes)";
  const std::string stream = w + "reads " + absent_why;
  const std::string past = w + "reads past " + row_name;
  // as d_cl_src resolves a source: the key, else the stored val
  auto fits = [&](u8 src, u32 off, u32 bytes) {
    return (u64)off + bytes <= (src == MZ_SRC_KEY ? 8ull * kw : (u64)vb);
  };
  for (u32 i = 0; i < cl->n_filters; i++) {
    const mz_gpu_filter &f = cl->filters[i];
    if (f.src == absent) return stream;
    u32 w = f.width == 4 ? 4 : 8;  // d_read_int
    if (f.src != MZ_SRC_COMPUTE) {
      if (!fits(f.src, f.off, w)) return past;
      continue;
    }
    if (f.arg0_src == absent || f.arg1_src == absent)
      return stream;
    if (f.off == MZ_COMPUTE_Q17_QTYLT &&  // i64; i128 sum + count at +24
        !(fits(f.arg0_src, f.arg0, 8) && fits(f.arg1_src, f.arg1, 32)))
      return past;
    if (f.off == MZ_COMPUTE_CMP_FIELDS &&
        !(fits(f.arg0_src, f.arg0, w) && fits(f.arg1_src, f.arg1, w)))
      return past;
  }
  for (int which = 0; which < 2; which++) {
    u32 nf = which ? cl->n_val_fields : cl->n_key_fields;
    const mz_gpu_field *fs = which ? cl->val_fields : cl->key_fields;
    u64 bytes = 0;
    for (u32 i = 0; i < nf; i++) {
      const mz_gpu_field &f = fs[i];
      if (f.src == absent) return stream;
      if (f.src == MZ_SRC_COMPUTE && f.off != MZ_COMPUTE_CONST0) {
        if (f.arg0_src == absent ||
            f.arg1_src == absent)
          return stream;
        if (!(fits(f.arg0_src, f.arg0, 8) && fits(f.arg1_src, f.arg1, 8)))
          return past;
      } else if (f.src != MZ_SRC_COMPUTE && !fits(f.src, f.off, f.width)) {
        return past;
      }
      bytes += f.src == MZ_SRC_COMPUTE ? 8 : f.width;  // computes are i64
    }
    if (bytes != (which ? (u64)cl->out.val_bytes : 8ull * cl->out.key_words))
      return w + "field widths do not add up to its out schema";
  }
  return std::string();
}

// ------------------------------------------------------------ peek select
// The kernels of mz_gpu_peek_select sit here, behind every kernel of the
// maintenance path, so that adding them leaves those kernels where they
// were in the code object.
// Key-range ends of every batch of a peek (mz_gpu_peek_select, range): one
// thread per (batch, side) binary-searches the batch's sorted keys for the
// first key at or beyond the bound (lo: the first key that passes; hi: the
// first that no longer does) and writes, per batch, out[4b + side] = that
// key's first val index and out[4b + 2 + side] = that val's first update
// index. kv_off has n_keys + 1 entries and vu_off n_vals + 1, so the end
// positions are in bounds.
__global__ void k_peek_range_bounds(BatchList bl, u32 kw,
                                    const mz_gpu_key_range r, u64 *out) {
  u32 t = threadIdx.x;
  if (t >= 2u * (u32)bl.n) return;
  const DevBatch &b = bl.b[t >> 1];
  u32 side = t & 1;
  u32 kind = side ? r.hi_kind : r.lo_kind;
  static_assert(MAX_KW == 2, "mz_gpu_key_range holds two words");
  i64 b0 = side ? r.hi[0] : r.lo[0], b1 = side ? r.hi[1] : r.lo[1];
  u64 idx = side ? b.n_keys : 0;
  if (kind != MZ_KB_UNBOUNDED) {
    // skip keys <= bound (strict) or < bound
    bool strict = side ? kind == MZ_KB_INCLUSIVE : kind == MZ_KB_EXCLUSIVE;
    u64 lo = 0, hi = b.n_keys;
    while (lo < hi) {
      u64 mid = lo + (hi - lo) / 2;
      const u64 *k = b.keys + mid * kw;
      i64 x = (i64)k[0], y = b0;
      if (x == y && kw > 1) x = (i64)k[1], y = b1;
      int c = x < y ? -1 : x > y ? 1 : 0;  // d_key_cmp against the bound
      if (strict ? c <= 0 : c < 0)
        lo = mid + 1;
      else
        hi = mid;
    }
    idx = lo;
  }
  u32 v = b.kv_off[idx];
  out[4 * (t >> 1) + side] = v;
  out[4 * (t >> 1) + 2 + side] = b.vu_off[v];
}

// Exact total of n positive i64 counts without a 128-bit atomic: sums[0]
// += the counts' high 32 bits, sums[1] += their low 32 bits. Fewer than
// 2^32 rows keep both sums exact in a u64 (peek_total_fits puts them
// together). One atomic pair per wave.
__global__ void k_peek_count_sums(const i64 *diffs, u64 n,
                                  unsigned long long *sums) {
  unsigned long long hi = 0, lo = 0;
  GRID_STRIDE(i, n) {
    u64 c = (u64)diffs[i];
    hi += c >> 32;
    lo += c & 0xFFFFFFFFull;
  }
  for (int d = 32; d; d >>= 1) {
    hi += __shfl_down(hi, d, 64);
    lo += __shfl_down(lo, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(sums, hi);
    atomicAdd(sums + 1, lo);
  }
}

// Order-preserving u64 radix key of one finishing order column for the row
// perm[i] (k_order_sortkey extended: key source, NULL rank, 16-byte datums).
// part 0 = the datum's word (of a 16-byte datum the biased high word),
// part 1 = the low word of a 16-byte datum, part 2 = the NULL rank: 1 for
// the side that sorts last. A NULL's datum key is 0 whatever its bytes
// hold; descending columns invert the datum keys, never the rank.
enum { PEEK_KEY_DATUM = 0, PEEK_KEY_LOW = 1, PEEK_KEY_NULL = 2 };
__global__ void k_peek_sortkey(const u64 *keys, u32 kw, const u8 *vals,
                               u32 vb, const u32 *perm, u64 *skey, u64 n,
                               const mz_gpu_peek_order oc, u32 part) {
  GRID_STRIDE(i, n) {
    u64 r = perm[i];
    bool null = oc.null_off != MZ_GPU_NO_NULL &&
                vals[r * vb + oc.null_off] != 0;
    u64 s = 0;
    if (part == PEEK_KEY_NULL) {
      s = null == (oc.nulls_last != 0) ? 1 : 0;
    } else if (!null) {
      const u64 sign = 0x8000000000000000ull;
      if (oc.src == MZ_SRC_KEY) {
        s = keys[r * kw + oc.off / 8] ^ sign;
      } else {
        const u8 *v = vals + r * vb + oc.off;
        if (oc.width == 4)
          s = (u64)(i64)(int32_t)(u32)le_val_word(v, 4) ^ sign;
        else if (oc.width == 8)
          s = le_val_word(v, 8) ^ sign;
        else
          s = part == PEEK_KEY_LOW ? le_val_word(v, 8)
                                   : le_val_word(v + 8, 8) ^ sign;
      }
      if (oc.desc) s = ~s;
    }
    skey[i] = s;
  }
}

// Copies of ordered row i inside the position window [off, end): the row
// occupies [pre[i] - c, pre[i]) of the expanded sequence (pre = inclusive
// scan of the ordered counts c; the total fits an i64, so nothing wraps).
__device__ __forceinline__ u64 d_peek_kept(const u64 *pre, const i64 *c,
                                           u64 i, u64 off, u64 end) {
  u64 hi = pre[i], lo = hi - (u64)c[i];
  u64 wlo = lo > off ? lo : off, whi = hi < end ? hi : end;
  return whi > wlo ? whi - wlo : 0;
}

__global__ void k_peek_kept_flags(const u64 *pre, const i64 *c, u64 n,
                                  u64 off, u64 end, u32 *flags) {
  GRID_STRIDE(i, n) flags[i] = d_peek_kept(pre, c, i, off, end) ? 1u : 0u;
}

// The finishing's clip (k_topk_kept's window, whole result as one group):
// ordered row i = source row perm[i] (perm == nullptr: row i) leaves with
// its kept copies at pos[i], its rank among the kept rows, so the out
// columns are in finishing order.
__global__ void k_peek_clip_emit(const u64 *keys, u32 kw, const u8 *vals,
                                 u32 vb, const u32 *perm, const i64 *c,
                                 const u64 *pre, const u32 *pos, u64 n,
                                 u64 off, u64 end, u64 t, u64 *okeys,
                                 u8 *ovals, u64 *otimes, i64 *odiffs) {
  GRID_STRIDE(i, n) {
    u64 kept = d_peek_kept(pre, c, i, off, end);
    if (!kept) continue;
    u64 r = perm ? perm[i] : i, o = pos[i];
    for (u32 w = 0; w < kw; w++) okeys[o * kw + w] = keys[r * kw + w];
    for (u32 b = 0; b < vb; b++) ovals[o * vb + b] = vals[r * vb + b];
    otimes[o] = t;
    odiffs[o] = (i64)kept;
  }
}

// Narrow a peek's batch snapshot to the vals of the in-range keys
// (mz_gpu_peek_select, range): k_peek_range_bounds finds every batch's two
// ends, one readback brings them to the host, and each DevBatch copy in
// `bl` is moved to its first in-range val. val_key and vu_off hold absolute
// indices, so keys, times and diffs stay where they are and k_scan_walk
// runs unchanged over the narrowed list.
static void peek_narrow_batchlist(Ctx *ctx, const mz_gpu_key_range *range,
                                  u32 kw, u32 vb, BatchList &bl) {
  if (bl.n == 0) return;
  u64 *dends = (u64 *)(*ctx->scr).get(4 * 12 * 8);
  hipLaunchKernelGGL(k_peek_range_bounds, dim3(1), dim3(64), 0, ctx->stream,
                     bl, kw, *range, dends);
  const u64 *e = (const u64 *)d2h_pinned(ctx, dends, 4 * 8 * (size_t)bl.n);
  for (int i = 0; i < bl.n; i++) {
    DevBatch &b = bl.b[i];
    u64 vlo = e[4 * i], vhi = std::max(e[4 * i + 1], vlo);  // lo > hi: empty
    u64 ulo = e[4 * i + 2], uhi = std::max(e[4 * i + 3], ulo);
    if (b.vals) b.vals += vlo * vb;
    b.val_key += vlo;
    b.vu_off += vlo;
    b.n_vals = vhi - vlo;
    b.n_upds = uhi - ulo;
  }
}

// The finishing of mz_gpu_peek_select over the n consolidated rows `o`
// (canonical order, counts > 0): exact total, stable radix passes from the
// last order column to the first (so ties keep the canonical order), exact
// scan of the ordered counts, in-order clip. Replaces o and n by the
// finished rows; returns the message on failure (o is then unchanged).
static std::string peek_finish(Ctx *ctx, const mz_gpu_finishing *fin, u32 kw,
                               u32 vb, u64 as_of, FlatCols &o, u64 &n) {
  auto &S = (*ctx->scr);
  if (n == 0) return "";
  unsigned long long *sums = (unsigned long long *)S.get(16);
  fill_u64(ctx, (u64 *)sums, 2, 0);
  hipLaunchKernelGGL(k_peek_count_sums, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, o.diffs, n, sums);
  const u64 *hs = (const u64 *)d2h_pinned(ctx, sums, 16);
  u64 total;
  if (!peek_total_fits(hs[0], hs[1], &total))
    return "peek_select: total multiplicity exceeds int64";
  if (peek_finishing_is_identity(fin)) return "";
  const u32 *perm = nullptr;
  const i64 *cnt = o.diffs;
  if (fin->n_order) {
    PermSort ps(ctx, n, 1);  // full-word and 1-bit NULL-rank passes
    auto pass = [&](const mz_gpu_peek_order &oc, u32 part) {
      hipLaunchKernelGGL(k_peek_sortkey, dim3(ngrid(n)), dim3(BLK), 0,
                         ctx->stream, o.keys, kw, o.vals, vb, ps.perm(),
                         ps.skey(), n, oc, part);
      ps.pass(part == PEEK_KEY_NULL ? 1 : 64);
    };
    for (int j = (int)fin->n_order - 1; j >= 0; j--) {
      const mz_gpu_peek_order &oc = fin->order[j];
      if (oc.src != MZ_SRC_KEY && oc.width == 16) pass(oc, PEEK_KEY_LOW);
      pass(oc, PEEK_KEY_DATUM);
      if (oc.null_off != MZ_GPU_NO_NULL) pass(oc, PEEK_KEY_NULL);
    }
    i64 *sd = (i64 *)S.get(n * 8);
    hipLaunchKernelGGL(k_gather_i64, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, o.diffs, ps.perm(), sd, n);
    perm = ps.perm();
    cnt = sd;
  }
  u64 *pre = (u64 *)S.get(n * 8);
  inclusive_scan_u64(ctx, (const u64 *)cnt, pre, n);
  u64 end = peek_window_end(fin->offset, fin->limit);
  u32 *flags = (u32 *)S.get(n * 4), *pos = (u32 *)S.get((n + 1) * 4);
  hipLaunchKernelGGL(k_peek_kept_flags, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, pre, cnt, n, fin->offset, end, flags);
  u64 K = exclusive_scan_u32(ctx, flags, pos, n);
  FlatCols f = flat_alloc(ctx, K, kw, vb);
  if (K)
    hipLaunchKernelGGL(k_peek_clip_emit, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, o.keys, kw, o.vals, vb, perm, cnt, pre,
                       pos, n, fin->offset, end, as_of, f.keys, f.vals,
                       f.times, f.diffs);
  flat_free(ctx, o);
  o = f;
  n = K;
  return "";
}

// Peek host path (mz_gpu_peek_scan; mz_gpu_peek_select adds a key range, a
// finishing and statistics): the probe protocol with
// k_scan_walk as the launch — prepare, snapshot, run_probe, consolidate,
// negative-count check, finishing, error stream. `who` prefixes the
// messages.
static int peek_scan_impl(Ctx *ctx, const char *who, mz_gpu_arr *arr,
                          u64 as_of, const mz_gpu_key_range *range,
                          const mz_gpu_closure *mfp,
                          const mz_gpu_finishing *fin, int allow_negative,
                          mz_gpu_peek_stats *stats, mz_gpu_out **out) {
  const std::string w = std::string(who) + ": ";
  if (is_varlen(arr->schema.vb)) {
    ctx->err = w + "varlen arrangements unsupported";
    return 1;
  }
  u32 kw = arr->schema.kw, vb = arr->schema.vb;
  mz_gpu_closure cl{};
  if (mfp) {
    std::string why = mfp_shape_error(
        who, mfp, kw, vb, MZ_SRC_VAL_STREAM,
        "MZ_SRC_VAL_STREAM (a scan has no stream side)",
        "the arrangement's key or val");
    if (!why.empty()) {
      ctx->err = why;
      return 1;
    }
    cl = *mfp;
  } else {  // identity: (key, val) as stored
    cl.n_key_fields = 1;
    cl.key_fields[0] = mz_gpu_field{MZ_SRC_KEY, 0, (u8)(8 * kw), 0, 0, 0, 0};
    cl.n_val_fields = vb ? 1u : 0u;
    if (vb)
      cl.val_fields[0] =
          mz_gpu_field{MZ_SRC_VAL_LOOKUP, 0, (u8)vb, 0, 0, 0, 0};
    cl.out.key_words = kw;
    cl.out.val_bytes = vb;
  }
  u32 okw = cl.out.key_words, ovb = cl.out.val_bytes;
  {
    std::string why = range ? peek_range_error(range, kw) : "";
    if (why.empty() && fin)
      why = peek_finishing_error(fin, okw, ovb, allow_negative);
    if (!why.empty()) {
      ctx->err = why;
      return 1;
    }
  }
  if (as_of == ~0ull) {  // as_of + 1 is the probe's exclusive bound
    ctx->err = w + "as_of out of range";
    return 1;
  }
  if (as_of < arr->logical_compaction) {
    ctx->err = w + "as_of " + std::to_string(as_of) +
               " is before the compaction frontier " +
               std::to_string(arr->logical_compaction);
    return 1;
  }
  if (stats) *stats = mz_gpu_peek_stats{0, 0};
  // a pending insert wholly beyond as_of keeps running on its lane
  probe_prepare(ctx, arr, PM_HALF_LE, as_of + 1);
  BatchList bl;
  build_probe_batchlist(ctx, arr, as_of + 1, bl);
  (*ctx->scr).reset();
  if (range) peek_narrow_batchlist(ctx, range, kw, vb, bl);
  ScanBases vbase;
  u64 n = 0, n_upds = 0;
  for (int b = 0; b < bl.n; b++) {
    vbase.v[b] = n;
    n += bl.b[b].n_vals;
    n_upds += bl.b[b].n_upds;
  }
  vbase.v[bl.n] = n;
  if (n == 0) {
    *out = empty_out(ctx, okw, ovb);
    return 0;
  }
  // One row per val at most: n is an exact bound on the ok queue, so only
  // the error queue can overflow into the exact relaunch.
  ProbeQueue pq{okw, ovb};
  ProbeCounts r =
      run_probe(ctx, pq, n, n / 4 + 1024, 2, n, [&](EmitQueue q) {
        hipLaunchKernelGGL(k_scan_walk, dim3(ngrid(n)), dim3(BLK), 0,
                           ctx->stream, bl, vbase, kw, vb, as_of, cl, q);
      });
  u64 M = r.M;
  if (ctx->time_kernels) {  // run_probe has synced and entered the call
    ctx->probe_batches += (u64)bl.n;
    // Algorithmic bytes of the scan, each touched once: per val its bytes
    // + val_key (4) + the vu_off pair (8) + its key; per update time +
    // diff (16); the emitted rows.
    ctx->probe_alg_bytes += n * (vb + 4ull + 8 + 8ull * kw) +
                            n_upds * 16ull + M * (8ull * okw + ovb + 16);
  }
  // the same (key, val) lives in several batches, and a projecting mfp
  // collapses distinct rows
  DevUpdates pin{pq.q.okeys, pq.q.ovals, pq.q.otimes, pq.q.odiffs, M};
  u64 Mc;
  FlatCols o = consolidate_dev(ctx, okw, ovb, pin, &Mc);
  pq.free_ok(ctx);
  if (!allow_negative && Mc) {
    u64 *dneg = (u64 *)(*ctx->scr).get(8);
    fill_u64(ctx, dneg, 1, 0);
    hipLaunchKernelGGL(k_any_negative, dim3(ngrid(Mc)), dim3(BLK), 0,
                       ctx->stream, o.diffs, Mc,
                       (unsigned long long *)dneg);
    u64 neg = *(u64 *)d2h_pinned(ctx, dneg, 8);
    if (neg) {
      flat_free(ctx, o);
      pq.free_errs(ctx);
      ctx->err = w + "negative multiplicity (" + std::to_string(neg) +
                 " rows)";
      return 1;
    }
  }
  if (stats) *stats = mz_gpu_peek_stats{n, Mc};
  if (fin) {
    std::string why = peek_finish(ctx, fin, okw, ovb, as_of, o, Mc);
    if (!why.empty()) {
      flat_free(ctx, o);
      pq.free_errs(ctx);
      ctx->err = why;
      return 1;
    }
  }
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = make_out(o, Mc, okw, ovb);
  attach_err_stream(ctx, *out, pq, r.E);
  return 0;
}

int mz_gpu_peek_scan(mz_gpu_ctx *c, mz_gpu_arr *arr, uint64_t as_of,
                     const mz_gpu_closure *mfp, int allow_negative,
                     mz_gpu_out **out) {
  return peek_scan_impl(&c->impl, "peek_scan", arr, as_of, nullptr, mfp,
                        nullptr, allow_negative, nullptr, out);
}

int mz_gpu_peek_select(mz_gpu_ctx *c, mz_gpu_arr *arr, uint64_t as_of,
                       const mz_gpu_key_range *range,
                       const mz_gpu_closure *mfp,
                       const mz_gpu_finishing *fin, int allow_negative,
                       mz_gpu_peek_stats *stats, mz_gpu_out **out) {
  return peek_scan_impl(&c->impl, "peek_select", arr, as_of, range, mfp, fin,
                        allow_negative, stats, out);
}

// ------------------------------------------------------ temporal filter
// The operator that owns future-stamped updates (mz_gpu.h):
// the held buffer is operator-owned flat columns of `cap` rows, the first
// n_held of them consolidated; min_time mirrors the smallest held time.
struct mz_gpu_temporal {
  mz_gpu_closure cl;  // the mfp, or the identity projection
  TemporalBounds tb;
  u32 kw, vb;         // input schema; the held rows have cl.out's
  FlatCols held;
  u64 cap = 0, n_held = 0;
  u64 min_time = ~0ull;
  u64 frontier = ~0ull;
  bool started = false;
};

static void temporal_free(Ctx *ctx, mz_gpu_temporal *op) {
  flat_free(ctx, op->held);
  delete op;
}

mz_gpu_temporal *mz_gpu_temporal_create(mz_gpu_ctx *c,
                                        const mz_gpu_temporal_spec *spec) {
  Ctx *ctx = &c->impl;
  auto fail = [&](const std::string &msg) -> mz_gpu_temporal * {
    ctx->err = msg;
    return nullptr;
  };
  u32 kw = spec->in.key_words, vb = spec->in.val_bytes;
  if (is_varlen(vb)) return fail("temporal: varlen vals unsupported");
  if (kw < 1 || kw > (u32)MAX_KW || vb > (u32)MAX_VB)
    return fail("temporal: in schema unsupported (1..2 key words, "
                "fixed-width val of at most 64 bytes)");
  if (spec->n_bounds < 1 || spec->n_bounds > MZ_GPU_MAX_BOUNDS)
    return fail("temporal: n_bounds must be 1.." +
                std::to_string(MZ_GPU_MAX_BOUNDS));
  for (u32 i = 0; i < spec->n_bounds; i++) {
    const mz_gpu_time_bound &b = spec->bounds[i];
    if (b.kind != MZ_TB_LOWER && b.kind != MZ_TB_UPPER)
      return fail("temporal: bound of unknown kind");
    if (b.src != MZ_SRC_KEY && b.src != MZ_SRC_VAL_STREAM)
      return fail("temporal: a bound reads MZ_SRC_KEY or MZ_SRC_VAL_STREAM");
    if (b.width != 4 && b.width != 8)
      return fail("temporal: bound width must be 4 or 8");
    if ((u64)b.off + b.width + (b.nullable ? 1 : 0) >
        (b.src == MZ_SRC_KEY ? 8ull * kw : (u64)vb))
      return fail("temporal: a bound reads past the input row's key or val");
  }
  mz_gpu_closure cl{};
  if (spec->has_mfp) {
    cl = spec->mfp;
    std::string why = mfp_shape_error(
        "temporal", &cl, kw, vb, MZ_SRC_VAL_LOOKUP,
        "MZ_SRC_VAL_LOOKUP (a temporal filter has no lookup side)",
        "the input row's key or val");
    if (!why.empty()) return fail(why);
    // d_cl_src sends every source but the key and the stream val to the
    // lookup side, which does not exist here
    auto row_src = [](u8 s) {
      return s == MZ_SRC_KEY || s == MZ_SRC_VAL_STREAM;
    };
    const char *src = "temporal: mfp reads a source other than the input row";
    for (u32 i = 0; i < cl.n_filters; i++) {
      const mz_gpu_filter &f = cl.filters[i];
      if (f.src == MZ_SRC_COMPUTE ? !(row_src(f.arg0_src) &&
                                      row_src(f.arg1_src))
                                  : !row_src(f.src))
        return fail(src);
    }
    for (int which = 0; which < 2; which++) {
      u32 nf = which ? cl.n_val_fields : cl.n_key_fields;
      const mz_gpu_field *fs = which ? cl.val_fields : cl.key_fields;
      for (u32 i = 0; i < nf; i++) {
        const mz_gpu_field &f = fs[i];
        if (f.src != MZ_SRC_COMPUTE) {
          if (!row_src(f.src)) return fail(src);
          continue;
        }
        if (f.off == MZ_COMPUTE_DIV_I64)
          return fail("temporal: the projection may not contain a field "
                      "that can error (MZ_COMPUTE_DIV_I64); put the "
                      "division in a following mz_gpu_map");
        if (f.off != MZ_COMPUTE_CONST0 &&
            !(row_src(f.arg0_src) && row_src(f.arg1_src)))
          return fail(src);
      }
    }
  } else {  // identity: (key, val) as they arrive
    cl.n_key_fields = 1;
    cl.key_fields[0] = mz_gpu_field{MZ_SRC_KEY, 0, (u8)(8 * kw), 0, 0, 0, 0};
    cl.n_val_fields = vb ? 1u : 0u;
    if (vb)
      cl.val_fields[0] =
          mz_gpu_field{MZ_SRC_VAL_STREAM, 0, (u8)vb, 0, 0, 0, 0};
    cl.out.key_words = kw;
    cl.out.val_bytes = vb;
  }
  mz_gpu_temporal *op = new mz_gpu_temporal();
  op->cl = cl;
  op->tb.n = spec->n_bounds;
  for (u32 i = 0; i < spec->n_bounds; i++) op->tb.b[i] = spec->bounds[i];
  op->tb.until = spec->until;
  op->kw = kw;
  op->vb = vb;
  // 64K rows by default; grows on demand
  op->cap = spec->initial_rows ? spec->initial_rows : (1ull << 16);
  op->held = flat_alloc(ctx, op->cap, cl.out.key_words, cl.out.val_bytes);
  ctx->temporals.push_back(op);
  return op;
}

void mz_gpu_temporal_drop(mz_gpu_ctx *c, mz_gpu_temporal *op) {
  auto &v = c->impl.temporals;
  v.erase(std::remove(v.begin(), v.end(), op), v.end());
  temporal_free(&c->impl, op);
}

int mz_gpu_temporal_stats(mz_gpu_ctx *, mz_gpu_temporal *op,
                          uint64_t *held_rows, uint64_t *next_time,
                          uint64_t *frontier) {
  *held_rows = op->n_held;
  *next_time = op->min_time;
  *frontier = op->started ? op->frontier : ~0ull;
  return 0;
}

// One push. Nothing of the operator's state is written before the input is
// known to be good: the kernels fill fresh queues (or the free tail of the
// held buffer), and the held buffer, its mirrors and the frontier change
// after the counter readback only.
//   stage -> k_temporal_eval -> k_temporal_release (if a held time is below
//   upper) -> counter readback -> consolidate ready rows (the out-batch) ->
//   consolidate held-kept + held-new (the new held buffer) -> closing
//   readback of its row count and smallest time -> error stream.
static int temporal_push_impl(Ctx *ctx, mz_gpu_temporal *op,
                              const mz_gpu_updates *u, mz_gpu_out **out) {
  if (is_varlen(op->vb) || u->val_offs) {
    ctx->err = "temporal: varlen updates unsupported";
    return 1;
  }
  if (op->started && u->lower != op->frontier) {
    ctx->err = "temporal: delta.lower " + std::to_string(u->lower) +
               " is not the operator's frontier " +
               std::to_string(op->frontier);
    return 1;
  }
  if (u->upper < u->lower) {
    ctx->err = "temporal: delta.upper is before delta.lower";
    return 1;
  }
  (*ctx->scr).reset();
  const mz_gpu_closure &cl = op->cl;
  u32 okw = cl.out.key_words, ovb = cl.out.val_bytes;
  u64 n = u->n, upper = u->upper;
  // the common case of a far-future window: no held time is due
  bool release = op->n_held && op->min_time < upper;
  auto advance = [&]() {
    op->started = true;
    op->frontier = upper;
  };
  if (n == 0 && !release) {  // a tick that releases nothing
    *out = empty_out(ctx, okw, ovb);
    advance();
    return 0;
  }
  if (op->n_held + 2 * n >= (1ull << 32)) {
    ctx->err = "temporal: held rows + 2 * delta rows must stay below 2^32";
    return 1;
  }
  // grow the held buffer to take this push's 2n rows behind what it holds
  if (op->n_held + 2 * n > op->cap) {
    u64 ncap = std::max<u64>(op->n_held + 2 * n, 2 * op->cap);
    FlatCols g = flat_alloc(ctx, ncap, okw, ovb);
    u64 m = op->n_held;
    if (m) {
      HIP_CHECK(hipMemcpyAsync(g.keys, op->held.keys, m * okw * 8,
                               hipMemcpyDeviceToDevice, ctx->stream));
      if (ovb)
        HIP_CHECK(hipMemcpyAsync(g.vals, op->held.vals, m * ovb,
                                 hipMemcpyDeviceToDevice, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(g.times, op->held.times, m * 8,
                               hipMemcpyDeviceToDevice, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(g.diffs, op->held.diffs, m * 8,
                               hipMemcpyDeviceToDevice, ctx->stream));
    }
    flat_free(ctx, op->held);
    op->held = g;
    op->cap = ncap;
  }
  // Queues at their exact bounds. Without a release pass the new held rows
  // go behind the resident ones, in place; with one, kept and new rows
  // both go to a fresh buffer.
  FlatCols work = release ? flat_alloc(ctx, op->cap, okw, ovb) : op->held;
  u64 held0 = release ? 0 : op->n_held;
  HeldQueue hq{op->cap, work.keys, work.vals, work.times, work.diffs};
  ProbeQueue pq{okw, ovb};
  pq.alloc(ctx, std::max<u64>(2 * n + (release ? op->n_held : 0), 1),
           std::max<u64>(n, 1));
  u64 *ctr = (u64 *)(*ctx->scr).get(8 * 6);
  pq.q.ctr = (unsigned long long *)ctr;
  // [0] ready [1] errors [2] held [3] bad input times; the closing
  // readback's [4] held rows after consolidation [5] their smallest time
  fill_u64(ctx, ctr, 5, 0);
  fill_u64(ctx, ctr + 2, 1, held0);
  fill_u64(ctx, ctr + 5, 1, ~0ull);
  if (n) {
    DevUpdates d = stage_updates(ctx, u, op->kw, op->vb);
    DeltaView dv{d.keys, op->vb ? d.vals : nullptr, op->vb, d.times, d.diffs,
                 n, op->kw};
    if (ctx->time_kernels) HIP_CHECK(hipEventRecord(ctx->ev_a, ctx->stream));
    hipLaunchKernelGGL(k_temporal_eval, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, dv, u->lower, upper, cl, op->tb, pq.q,
                       hq);
    if (ctx->time_kernels) HIP_CHECK(hipEventRecord(ctx->ev_b, ctx->stream));
  }
  if (release)
    hipLaunchKernelGGL(k_temporal_release, dim3(ngrid(op->n_held)),
                       dim3(BLK), 0, ctx->stream, op->held.keys,
                       op->held.vals, op->held.times, op->held.diffs,
                       op->n_held, okw, ovb, upper, pq.q, hq);
  u64 h[4];
  memcpy(h, d2h_pinned(ctx, ctr, 8 * 4), sizeof h);
  u64 R = h[0], E = h[1], H = h[2], bad = h[3];
  if (n && ctx->time_kernels) {  // the readback synced
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b));
    ctx->probe_ms += ms;
    ctx->probe_rows += n;
    ctx->probe_launches += 1;
  }
  if (bad) {  // state untouched: only free memory was written
    pq.free(ctx);
    if (release) flat_free(ctx, work);
    ctx->err = "temporal: " + std::to_string(bad) +
               " input times outside [delta.lower, delta.upper)";
    return 1;
  }
  // the out-batch: everything below upper, from this delta and from held
  if (R) {
    DevUpdates rin{pq.q.okeys, pq.q.ovals, pq.q.otimes, pq.q.odiffs, R};
    u64 Rc;
    FlatCols o = consolidate_dev(ctx, okw, ovb, rin, &Rc);
    *out = make_out(o, Rc, okw, ovb);
  } else {
    *out = empty_out(ctx, okw, ovb);
  }
  pq.free_ok(ctx);
  // the new held buffer. Without a release pass and without new held rows
  // it is the old one, untouched.
  if (release || H > held0) {
    FlatCols nh = flat_alloc(ctx, op->cap, okw, ovb);
    if (H) {
      DevUpdates hin{work.keys, work.vals, work.times, work.diffs, H};
      consolidate_core(ctx, okw, ovb, hin, nh, ctr + 4);
      hipLaunchKernelGGL(k_time_min, dim3(ngrid(H)), dim3(BLK), 0,
                         ctx->stream, nh.times, ctr + 4,
                         (unsigned long long *)(ctr + 5));
    }
    memcpy(h, d2h_pinned(ctx, ctr + 4, 8 * 2), 16);  // the closing readback
    if (release) flat_free(ctx, work);
    flat_free(ctx, op->held);
    op->held = nh;
    op->n_held = h[0];
    op->min_time = h[1];
  }
  attach_err_stream(ctx, *out, pq, E);
  advance();
  return 0;
}

int mz_gpu_temporal_push(mz_gpu_ctx *c, mz_gpu_temporal *op,
                         const mz_gpu_updates *delta, mz_gpu_out **out) {
  return temporal_push_impl(&c->impl, op, delta, out);
}

// Raw variant: output left unconsolidated (consumer consolidates).
int mz_gpu_halfjoin_raw(mz_gpu_ctx *c, mz_gpu_arr *lookup,
                        const mz_gpu_updates *delta,
                        uint32_t stream_val_bytes, int le,
                        const mz_gpu_closure *cl, mz_gpu_out **out) {
  return probe_impl(&c->impl, lookup, delta, stream_val_bytes,
                    le ? PM_HALF_LE : PM_HALF_LT, 0, cl, 0, out);
}

// Fused two-stage delta path (k_probe_path2): delta -> lookup1 (le1) ->
// lookup2 (le2), raw (unconsolidated) output with the err stream
// attached. The render layer uses this when a DeltaPathPlan has exactly
// two local stages; semantics identical to two mz_gpu_halfjoin_raw
// calls with the intermediate consolidation deferred (every consumer
// consolidates).
int mz_gpu_halfjoin2(mz_gpu_ctx *c, mz_gpu_arr *lk1, int le1,
                     const mz_gpu_closure *cl1, mz_gpu_arr *lk2, int le2,
                     const mz_gpu_closure *cl2, const mz_gpu_updates *u,
                     uint32_t stream_vb, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  if (is_varlen(lk1->schema.vb) || is_varlen(lk2->schema.vb)) {
    ctx->err = "halfjoin2: varlen lookups unsupported (use halfjoin)";
    return 1;
  }
  if (cl1->out.key_words == 0 || cl1->out.key_words > P2_MAX_KW ||
      cl1->out.val_bytes > P2_MAX_VB ||
      cl1->out.key_words != lk2->schema.kw) {
    ctx->err = "halfjoin2: stage-1 closure output shape unsupported";
    return 1;
  }
  int mode1 = le1 ? PM_HALF_LE : PM_HALF_LT;
  int mode2 = le2 ? PM_HALF_LE : PM_HALF_LT;
  probe_prepare(ctx, lk1, mode1, u->upper);
  probe_prepare(ctx, lk2, mode2, u->upper);
  BatchList bl1, bl2;
  build_probe_batchlist(ctx, lk1, u->lower, bl1);
  build_probe_batchlist(ctx, lk2, u->lower, bl2);
  (*ctx->scr).reset();
  u32 kw = lk1->schema.kw, lvb1 = lk1->schema.vb, lvb2 = lk2->schema.vb;
  u32 okw = cl2->out.key_words, ovb = cl2->out.val_bytes;
  DevUpdates d = stage_updates(ctx, u, kw, stream_vb);
  u64 n = d.n;
  if (n == 0 || bl1.n == 0 || bl2.n == 0) {
    *out = empty_out(ctx, okw, ovb);
    return 0;
  }
  u64 cap = (lk1->path_cap_hint ? lk1->path_cap_hint + 1 : 2) * n + 1024;
  DeltaView dv{d.keys, d.vals, stream_vb, d.times, d.diffs, n, kw};
  ProbeQueue pq{okw, ovb};
  // counters: [0] ok, [1] err, [2] intermediates
  ProbeCounts r =
      run_probe(ctx, pq, cap, n / 4 + 1024, 3, n, [&](EmitQueue q) {
        hipLaunchKernelGGL(k_probe_path2, dim3(ngrid(n * (u64)bl1.n)),
                           dim3(BLK), 0, ctx->stream, dv, lvb1, bl1, mode1,
                           *cl1, lvb2, bl2, mode2, *cl2, q);
      });
  u64 M = r.M, I = r.I;
  lk1->path_cap_hint = (M + n - 1) / n;
  if (ctx->time_kernels) {  // run_probe has synced and entered the call
    ctx->probe_batches += (u64)bl1.n + (u64)bl2.n;
    // algorithmic bytes: delta tuple + one hash line per stage-1 batch
    // + matched stage-1 val/upds + one hash line per stage-2 batch per
    // intermediate + matched stage-2 val/upds + output write. The
    // intermediate tuple itself stays in registers (never HBM).
    ctx->probe_alg_bytes +=
        n * (8ull * kw + stream_vb + 16) + n * 64ull * (u64)bl1.n +
        I * (lvb1 + 16ull) + I * 64ull * (u64)bl2.n +
        M * (lvb2 + 16ull) + M * (8ull * okw + ovb + 16);
  }
  *out = make_out(pq.q.okeys, pq.q.ovals, pq.q.otimes, pq.q.odiffs, M, okw,
                  ovb);
  attach_err_stream(ctx, *out, pq, r.E);
  return 0;
}

mz_gpu_red *mz_gpu_reduce_create(mz_gpu_ctx *c,
                                 const mz_gpu_reduce_spec *spec) {
  Ctx *ctx = &c->impl;
  if (is_varlen(spec->in.val_bytes) || is_varlen(spec->out.val_bytes)) {
    ctx->err = "varlen vals unsupported in reduce";
    return nullptr;
  }
  if (spec->n_aggs > MZ_GPU_MAX_AGGS) {
    ctx->err = "reduce: n_aggs out of range";
    return nullptr;
  }
  for (u32 a = 0; a < spec->n_aggs; a++)
    if (spec->aggs[a].func > MZ_AGG_SUM_F64) {
      // k_reduce_apply's last branch would silently treat it as SUM_F64
      ctx->err = "reduce: accumulable aggregates only (COUNT/SUM); MIN/MAX "
                 "go through mz_gpu_collation_create";
      return nullptr;
    }
  for (u32 a = 0; a < spec->n_aggs; a++)
    if (const char *msg = distinct_agg_error(spec->aggs[a], spec->in)) {
      ctx->err = std::string("reduce: ") + msg;
      return nullptr;
    }
  mz_gpu_red *r = new mz_gpu_red();
  r->spec = *spec;
  u32 kw = spec->in.key_words;
  // 4M keys default; grows on demand (kt_reserve); env override for
  // tests/tuning. Pair tables [key kw][datum][count] start at the same size.
  u64 cap = kt_env_cap("MZ_GPU_RED_CAP", 1ull << 22);
  for (u32 a = 0; a < spec->n_aggs; a++)
    if (agg_is_distinct(spec->aggs[a])) r->dist_agg[r->n_dist++] = a;
  r->d_ctr = dnew<u64>(ctx, 2 + r->n_dist);
  fill_u64(ctx, r->d_ctr, 2 + r->n_dist, 0);
  kt_create_at(ctx, r->tbl, kw, 1 + 6 * spec->n_aggs, cap, r->d_ctr,
               r->d_ctr + 1);
  for (u32 j = 0; j < r->n_dist; j++)
    kt_create_at(ctx, r->ptbl[j], kw + 1, 1, cap, r->d_ctr + 2 + j,
                 r->d_ctr + 1);
  c->impl.reds.push_back(r);
  return r;
}

void mz_gpu_reduce_drop(mz_gpu_ctx *c, mz_gpu_red *r) {
  Ctx *ctx = &c->impl;
  red_free_state(ctx, r);
  auto &v = ctx->reds;
  v.erase(std::remove(v.begin(), v.end(), r), v.end());
  delete r;
}

// Internal: reduce over already-staged device updates.
static int reduce_push_dev_impl(Ctx *ctx, mz_gpu_red *op, DevUpdates d,
                                u64 lower, u64 upper, mz_gpu_out **out);

int mz_gpu_reduce_push(mz_gpu_ctx *c, mz_gpu_red *op,
                       const mz_gpu_updates *u, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  return reduce_push_dev_impl(ctx, op, d, u->lower, u->upper, out);
}

// Concatenate two update streams (device-side) and reduce them as ONE
// logical batch — the render layer's path-output concat without a host
// round trip (reduce corrections depend on the combined batch, so the
// two streams must enter one push).
int mz_gpu_reduce_push2(mz_gpu_ctx *c, mz_gpu_red *op,
                        const mz_gpu_updates *u1, const mz_gpu_updates *u2,
                        mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  auto &S = (*ctx->scr);
  u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  DevUpdates d1 = stage_updates(ctx, u1, kw, vb);
  DevUpdates d2 = stage_updates(ctx, u2, kw, vb);
  u64 n = d1.n + d2.n;
  u64 capn = std::max<u64>(n, 1);
  u64 *k = (u64 *)S.get(capn * kw * 8);
  u8 *v = (u8 *)S.get(std::max<u64>(capn * vb, 1));
  u64 *t = (u64 *)S.get(capn * 8);
  i64 *df = (i64 *)S.get(capn * 8);
  if (n)
    hipLaunchKernelGGL(k_concat_updates, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, d1.keys, d1.vals, d1.times, d1.diffs,
                       d1.n, d2.keys, d2.vals, d2.times, d2.diffs, d2.n, kw,
                       vb, k, v, t, df);
  DevUpdates d{k, v, t, df, n};
  return reduce_push_dev_impl(ctx, op, d,
                              std::min(u1->lower, u2->lower),
                              std::max(u1->upper, u2->upper), out);
}

static int reduce_push_dev_impl(Ctx *ctx, mz_gpu_red *op, DevUpdates d,
                                u64 lower, u64 upper, mz_gpu_out **out) {
  auto &S = (*ctx->scr);
  u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  u32 okw = op->spec.out.key_words, ovb = op->spec.out.val_bytes;
  u64 n = d.n;
  // worst case every update opens a new group (and a new pair)
  kt_reserve(ctx, op->tbl, n);
  for (u32 j = 0; j < op->n_dist; j++) kt_reserve(ctx, op->ptbl[j], n);
  if (n == 0) {
    *out = empty_out(ctx, okw, ovb);
    return 0;
  }
  SortedCols s = sort_gather(ctx, d.keys, kw, d.vals, vb, d.times, d.diffs, n);
  std::vector<TimeSlice> slices = time_slices(ctx, s.times, n, lower, upper);
  // capacity 2 * n corrections max (each input row can change at most one
  // key per slice; 2 rows per changed key per slice)
  CorrBuf cb = corr_alloc(ctx, 2 * n + 16, okw, ovb);
  // A single-time push emits in canonical order (emit_old_new's ordered
  // form): two staging slots per group, compacted into cb after the apply.
  // Across several times the canonical order is key-major, so those pushes
  // keep the reservation and corr_finish's sort.
  bool ordered = upper == lower + 1;
  CorrBuf em = cb;  // where the apply kernel writes
  u32 *gcount = nullptr;
  if (ordered) {
    em.pk = (u64 *)S.get(2 * n * okw * 8);
    em.pv = (u8 *)S.get(std::max<u64>(2 * n * ovb, 1));
    em.pt = (u64 *)S.get(2 * n * 8);
    em.pd = (i64 *)S.get(2 * n * 8);
    gcount = (u32 *)S.get(n * 4);
  }
  // DISTINCT aggregates: the (key, datum) stream of each, sorted by
  // (time, key, datum). NULL datums stay as neutral rows, so the sorted
  // times equal s.times and the slices below cut both streams alike.
  u32 kw2 = kw + 1;  // pair tables' combined key: [key words][datum]
  u64 *psk[MZ_GPU_MAX_AGGS];
  i64 *psd[MZ_GPU_MAX_AGGS];
  for (u32 j = 0; j < op->n_dist; j++) {
    u64 *ck = (u64 *)S.get(n * kw2 * 8);
    i64 *pdf = (i64 *)S.get(n * 8);
    hipLaunchKernelGGL(k_pair_project, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, d.keys, kw, d.vals, vb, d.diffs, n,
                       op->spec.aggs[op->dist_agg[j]], ck, pdf);
    u32 *pperm = (u32 *)S.get(n * 4);
    sort_updates(ctx, ck, kw2, nullptr, 0, d.times, n, pperm, true);
    psk[j] = (u64 *)S.get(n * kw2 * 8);
    psd[j] = (i64 *)S.get(n * 8);
    hipLaunchKernelGGL(k_gather_keyrows, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, ck, kw2, pperm, psk[j], n);
    hipLaunchKernelGGL(k_gather_i64, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, pdf, pperm, psd[j], n);
  }
  for (auto [lo, hi, t] : slices) {
    u64 m = hi - lo;
    // Pair stage: fold the slice into each pair table and leave one
    // presence delta per (key, datum) group for the key stage, which runs
    // in a later launch than every pair apply it reads.
    PairViews pvs{};
    for (u32 j = 0; j < op->n_dist; j++) {
      const KeyedTable &P = op->ptbl[j];
      const u64 *pck = psk[j] + lo * kw2;
      Groups pg = group_sorted(ctx, pck, kw2, s.times + lo, m);
      Upsert pu = kt_upsert(ctx, P, pck, pg, m);
      int *pdelta = (int *)S.get(m * 4);
      hipLaunchKernelGGL(k_pair_apply, dim3(ngrid(m)), dim3(BLK), 0,
                         ctx->stream, psd[j] + lo, pg.starts, pg.gid, m, P.st,
                         pu.found, pu.miss, pu.misspos, P.d_nrows, pdelta);
      kt_commit(ctx, P, pu, pg, m);
      pvs.v[op->dist_agg[j]] = PairView{pck, pg.starts, pg.gid, pdelta};
    }
    // Key stage
    const u64 *sk = s.keys + lo * kw;
    Groups g = group_sorted(ctx, sk, kw, s.times + lo, m);
    Upsert up = kt_upsert(ctx, op->tbl, sk, g, m);
    if (op->n_dist)
      hipLaunchKernelGGL(k_reduce_apply_distinct, dim3(ngrid(m)), dim3(BLK),
                         0, ctx->stream, sk, s.vals + lo * vb, kw, vb,
                         s.diffs + lo, g.starts, g.gid, m, t, op->tbl.st,
                         up.found, up.miss, up.misspos, op->tbl.d_nrows,
                         op->spec, pvs, em.pk, em.pv, em.pt, em.pd,
                         em.ocount, gcount);
    else
      hipLaunchKernelGGL(k_reduce_apply, dim3(ngrid(m)), dim3(BLK), 0,
                         ctx->stream, sk, s.vals + lo * vb, kw, vb,
                         s.diffs + lo, g.starts, g.gid, m, t, op->tbl.st,
                         up.found, up.miss, up.misspos, op->tbl.d_nrows,
                         op->spec, em.pk, em.pv, em.pt, em.pd, em.ocount,
                         gcount);
    kt_commit(ctx, op->tbl, up, g, m);
    if (ordered) {  // the one slice: m == n
      PairCountIn pc{gcount, g.gid, m};
      u32 *pos = (u32 *)S.get((m + 1) * 4);
      auto it = rocprim::make_transform_iterator(
          rocprim::make_counting_iterator<u64>(0), pc);
      size_t need = 0;
      (void)rocprim::exclusive_scan(nullptr, need, it, pos, 0u, m + 1,
                                    rocprim::plus<u32>(), ctx->stream);
      void *tmp = S.get(need);
      (void)rocprim::exclusive_scan(tmp, need, it, pos, 0u, m + 1,
                                    rocprim::plus<u32>(), ctx->stream);
      hipLaunchKernelGGL(k_compact_pairs, dim3(ngrid(m)), dim3(BLK), 0,
                         ctx->stream, em.pk, em.pv, em.pt, em.pd, pc, pos, okw,
                         ovb, cb.pk, cb.pv, cb.pt, cb.pd, cb.ocount);
    }
  }
  // count + the whole counter block [key rows][err][pair rows] at once
  const u64 *h = corr_read(ctx, cb, op->d_ctr, 2 + op->n_dist);
  u64 emitted = h[0], errflag = h[2];
  op->tbl.n_rows = h[1];
  for (u32 j = 0; j < op->n_dist; j++) op->ptbl[j].n_rows = h[3 + j];
  mz_gpu_out *o;
  if (!ordered) {
    o = corr_finish(ctx, cb, emitted, errflag != 0);
  } else if (errflag) {
    corr_free(ctx, cb);
    o = nullptr;
  } else {  // already consolidated: cb's columns become the result
    o = make_out(cb.pk, cb.pv, cb.pt, cb.pd, emitted, okw, ovb);
  }
  if (errflag) {
    ctx->err = "reduce state capacity exceeded";
    return -1;
  }
  *out = o;
  return 0;
}

mz_gpu_thr *mz_gpu_threshold_create(mz_gpu_ctx *c, const mz_gpu_schema *s) {
  Ctx *ctx = &c->impl;
  if (is_varlen(s->val_bytes)) {
    ctx->err = "varlen vals unsupported in threshold";
    return nullptr;
  }
  (*ctx->scr).reset();
  mz_gpu_thr *r = new mz_gpu_thr();
  r->s = *s;
  r->kw2 = s->key_words + (s->val_bytes + 7) / 8;
  // 2M (key,val) pairs default; grows on demand; payload = the net count
  kt_create(ctx, r->tbl, r->kw2, 1, kt_env_cap("MZ_GPU_THR_CAP", 1ull << 21));
  return r;
}

void mz_gpu_threshold_drop(mz_gpu_ctx *c, mz_gpu_thr *r) {
  Ctx *ctx = &c->impl;
  kt_free(ctx, r->tbl);
  delete r;
}

int mz_gpu_threshold_push(mz_gpu_ctx *c, mz_gpu_thr *op,
                          const mz_gpu_updates *u, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  auto &S = (*ctx->scr);
  u32 kw = op->s.key_words, vb = op->s.val_bytes, kw2 = op->kw2;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  u64 n = d.n;
  kt_reserve(ctx, op->tbl, n);
  if (n == 0) {
    *out = empty_out(ctx, kw, vb);
    return 0;
  }
  u64 *ck = (u64 *)S.get(n * kw2 * 8);
  hipLaunchKernelGGL(k_pack_combined, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, d.keys, kw, vb ? d.vals : nullptr, vb, n,
                     ck, kw2);
  // sorted by (time, combined key)
  SortedCols s = sort_gather(ctx, ck, kw2, nullptr, 0, d.times, d.diffs, n);
  std::vector<TimeSlice> slices =
      time_slices(ctx, s.times, n, u->lower, u->upper);
  CorrBuf cb = corr_alloc(ctx, n + 16, kw, vb);  // ≤1 row per group per slice
  for (auto [lo, hi, t] : slices) {
    u64 m = hi - lo;
    const u64 *sk = s.keys + lo * kw2;
    Groups g = group_sorted(ctx, sk, kw2, s.times + lo, m);
    Upsert up = kt_upsert(ctx, op->tbl, sk, g, m);
    hipLaunchKernelGGL(k_threshold_apply, dim3(ngrid(m)), dim3(BLK), 0,
                       ctx->stream, sk, kw2, s.diffs + lo, g.starts, g.gid, m,
                       t, op->tbl.st, up.found, up.miss, up.misspos,
                       op->tbl.d_nrows, kw, vb, cb.pk, cb.pv, cb.pt, cb.pd,
                       cb.ocount);
    kt_commit(ctx, op->tbl, up, g, m);
  }
  const u64 *h = corr_read(ctx, cb, op->tbl.d_nrows, 2);  // [rows][err]
  u64 emitted = h[0], errflag = h[2];
  op->tbl.n_rows = h[1];
  mz_gpu_out *o = corr_finish(ctx, cb, emitted, errflag != 0);
  if (errflag) {
    ctx->err = "threshold state capacity exceeded";
    return -1;
  }
  *out = o;
  return 0;
}

// One eval set (a consolidated (key,val,net) snapshot of the changed
// groups, pe->n >= 1 rows) ordered by (group, order columns, canonical val
// tie-break), in scratch: the ordered columns, the key groups and the
// inclusive scan of the diffs. Stable LSD radix passes: order columns
// least-significant first, then key words to regroup (compare_columns +
// Row-order tie-break restatement, top_k.rs:733-766).
struct OrderedSnap {
  u64 *keys;
  u8 *vals;
  i64 *diffs;
  Groups g;
  u64 *pre;
};
static OrderedSnap order_snapshot(Ctx *ctx, u32 kw, u32 vb, u32 n_order,
                                  const mz_gpu_order_col *order,
                                  mz_gpu_out *pe) {
  u64 n = pe->n;
  auto &S = (*ctx->scr);
  const u64 *keys = (const u64 *)pe->keys;
  const u8 *vals = (const u8 *)pe->vals;
  const i64 *diffs = (const i64 *)pe->diffs;
  PermSort ps(ctx, n);
  for (int j = (int)n_order - 1; j >= 0; j--) {
    const mz_gpu_order_col &oc = order[j];
    hipLaunchKernelGGL(k_order_sortkey, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, vals, vb, ps.perm(), ps.skey(), n,
                       (u32)oc.off, (u32)oc.width, (u32)oc.desc);
    ps.pass();
  }
  for (int w = (int)kw - 1; w >= 0; w--) {
    hipLaunchKernelGGL(k_sortkey_key, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, keys, kw, (u32)w, ps.perm(), ps.skey(), n,
                       (u64)0, (u32 *)nullptr);
    ps.pass();
  }
  const u32 *perm = ps.perm();
  u64 *sk2 = (u64 *)S.get(n * kw * 8);
  u8 *sv2 = (u8 *)S.get(std::max<u64>(n * vb, 1));
  i64 *sd2 = (i64 *)S.get(n * 8);
  hipLaunchKernelGGL(k_gather_keyrows, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, keys, kw, perm, sk2, n);
  if (vb)
    hipLaunchKernelGGL(k_gather_valrows, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, vals, vb, perm, sv2, n);
  hipLaunchKernelGGL(k_gather_i64, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, diffs, perm, sd2, n);
  // eval rows all carry time t (the peek probe's join time)
  Groups g = group_sorted(ctx, sk2, kw, (const u64 *)pe->times, n);
  u64 *pre = (u64 *)S.get(n * 8);
  inclusive_scan_u64(ctx, (const u64 *)sd2, pre, n);
  return {sk2, sv2, sd2, g, pre};
}

// Order one eval set, compute each row's kept multiplicity window and
// append corrections with the given sign.
static void topk_eval_emit(Ctx *ctx, mz_gpu_topk *op, mz_gpu_out *pe,
                           u64 t, i64 sign, const FlatCols &p,
                           unsigned long long *ocount) {
  u64 n = pe->n;
  if (!n) return;
  u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  hipLaunchKernelGGL(k_check_pos, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     (const i64 *)pe->diffs, n, op->d_err);
  OrderedSnap s =
      order_snapshot(ctx, kw, vb, op->spec.n_order, op->spec.order, pe);
  hipLaunchKernelGGL(k_topk_kept, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     s.keys, kw, s.vals, vb, s.diffs, s.pre, s.g.starts,
                     s.g.gid, n, op->spec.offset, (i64)op->spec.limit, t,
                     sign, p.keys, p.vals, p.times, p.diffs, ocount);
}

mz_gpu_topk *mz_gpu_topk_create(mz_gpu_ctx *c, const mz_gpu_topk_spec *spec) {
  Ctx *ctx = &c->impl;
  mz_gpu_topk *r = new mz_gpu_topk();
  r->spec = *spec;
  r->arr = mz_gpu_arr_create(c, &spec->in);
  r->d_err = dnew<u64>(ctx, 1);
  fill_u64(ctx, r->d_err, 1, 0);
  return r;
}

void mz_gpu_topk_drop(mz_gpu_ctx *c, mz_gpu_topk *op) {
  mz_gpu_arr_drop(c, op->arr);  // owned group-contents arrangement
  dfree(&c->impl, op->d_err);
  delete op;
}

int mz_gpu_topk_push(mz_gpu_ctx *c, mz_gpu_topk *op,
                     const mz_gpu_updates *u, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  const u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  // each snapshot row emits at most one correction, appended through
  // *ocount into a zero-filled segment: the unused rows consolidate away
  auto eval = [&](u64 t, mz_gpu_out *oldp, mz_gpu_out *newp, SnapSeg *seg) {
    u64 capn = oldp->n + newp->n;
    if (!capn) return true;
    seg->cols = flat_alloc(ctx, capn, kw, vb);
    seg->n = capn;
    const FlatCols &p = seg->cols;
    fill_u64(ctx, p.keys, capn * kw, 0);
    fill_u8(ctx, p.vals, std::max<u64>(capn * vb, 1), 0);
    fill_u64(ctx, p.times, capn, 0);
    fill_u64(ctx, (u64 *)p.diffs, capn, 0);
    unsigned long long *ocount =
        (unsigned long long *)(*ctx->scr).get(8);
    fill_u64(ctx, (u64 *)ocount, 1, 0);
    topk_eval_emit(ctx, op, oldp, t, -1, p, ocount);
    topk_eval_emit(ctx, op, newp, t, +1, p, ocount);
    return true;
  };
  auto errors = [&](u64) -> const char * {
    return *(const u64 *)d2h_pinned(ctx, op->d_err, 8)
               ? "negative multiplicities in TopK"
               : nullptr;
  };
  return snapshot_diff_push(c, op->arr, vb, UINT64_MAX, u, eval, errors, out);
}

// ------------------------------------------------------ window functions

// The create-time rules (window_spec_error) are in window_spec.h.

mz_gpu_window *mz_gpu_window_create(mz_gpu_ctx *c,
                                    const mz_gpu_window_spec *spec) {
  Ctx *ctx = &c->impl;
  std::string why = window_spec_error(spec);
  if (!why.empty()) {
    ctx->err = "window: " + why;
    return nullptr;
  }
  mz_gpu_window *r = new mz_gpu_window();
  r->spec = *spec;
  for (u32 f = 0; f < spec->n_funcs; f++) {
    r->expand |= wf_expands(spec->funcs[f]);
    r->has_agg |= wf_is_agg(spec->funcs[f].func);
    r->has_sum |= spec->funcs[f].func == MZ_WF_SUM;
  }
  r->arr = mz_gpu_arr_create(c, &spec->in);
  r->d_err = dnew<u64>(ctx, 3);
  fill_u64(ctx, r->d_err, 3, 0);
  return r;
}

void mz_gpu_window_drop(mz_gpu_ctx *c, mz_gpu_window *op) {
  mz_gpu_arr_drop(c, op->arr);  // owned partition-contents arrangement
  dfree(&c->impl, op->d_err);
  delete op;
}

// The aggregates' prefix structures over one ordered snapshot, in scratch:
// per SUM datum the wrapping 128-bit prefix of m x, per nullable datum the
// prefix of m [non-NULL], per MIN / MAX the extremum scanned by partition
// from whichever end of the partition its frame is anchored at. Functions
// over the same datum share them.
static WinAggs window_agg_prefixes(Ctx *ctx, const mz_gpu_window_spec &sp,
                                   const OrderedSnap &s, u64 n) {
  auto &S = (*ctx->scr);
  const u32 vb = sp.in.val_bytes;
  WinAggs A{};
  u32 *rgid = nullptr;
  auto same_datum = [&](u32 f, u32 g) {
    const mz_gpu_window_func &a = sp.funcs[f], &b = sp.funcs[g];
    return wf_is_agg(b.func) && a.off == b.off && a.width == b.width &&
           !a.nullable == !b.nullable;
  };
  for (u32 f = 0; f < sp.n_funcs; f++) {
    const mz_gpu_window_func &fn = sp.funcs[f];
    if (!wf_is_agg(fn.func)) continue;
    const bool want_w = fn.func == MZ_WF_SUM;
    const bool want_c = fn.nullable != 0;  // COUNT(*) has no null byte
    for (u32 g = 0; g < f; g++) {
      if (!same_datum(f, g)) continue;
      if (want_w && !A.w[f]) A.w[f] = A.w[g];
      if (want_c && !A.c[f]) A.c[f] = A.c[g];
    }
    U128 *wt = want_w && !A.w[f] ? (U128 *)S.get(n * 16) : nullptr;
    u64 *ct = want_c && !A.c[f] ? (u64 *)S.get(n * 8) : nullptr;
    if (wt || ct)
      hipLaunchKernelGGL(k_window_sum_terms, dim3(ngrid(n)), dim3(BLK), 0,
                         ctx->stream, s.vals, vb, s.diffs, (u32)fn.off,
                         (u32)fn.width, (u32)fn.nullable, n, wt, ct);
    if (wt) {
      U128 *w = (U128 *)S.get(n * 16);
      size_t need = 0;
      (void)rocprim::inclusive_scan(nullptr, need, wt, w, n, U128Add(),
                                    ctx->stream);
      void *tmp = S.get(need);
      (void)rocprim::inclusive_scan(tmp, need, wt, w, n, U128Add(),
                                    ctx->stream);
      A.w[f] = w;
    }
    if (ct) {
      u64 *c = (u64 *)S.get(n * 8);
      inclusive_scan_u64(ctx, ct, c, n);
      A.c[f] = c;
    }
    if (fn.func != MZ_WF_MIN && fn.func != MZ_WF_MAX) continue;
    const bool is_max = fn.func == MZ_WF_MAX;
    A.sfx[f] = fn.frame == MZ_WF_FRAME_ROWS &&
               wf_end_kind(fn) == MZ_WB_UNBOUNDED_FOLLOWING &&
               wf_start_kind(fn) != MZ_WB_UNBOUNDED_PRECEDING;
    for (u32 g = 0; g < f && !A.x[f]; g++)
      if (same_datum(f, g) && sp.funcs[g].func == fn.func &&
          A.sfx[g] == A.sfx[f])
        A.x[f] = A.x[g];
    if (A.x[f]) continue;
    i64 *xt = (i64 *)S.get(n * 8), *x = (i64 *)S.get(n * 8);
    if (A.sfx[f] && !rgid) rgid = (u32 *)S.get(n * 4);
    hipLaunchKernelGGL(k_window_ext_terms, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, s.vals, vb, s.g.gid, (u32)fn.off,
                       (u32)fn.width, (u32)fn.nullable, is_max ? 1 : 0,
                       A.sfx[f] ? 1 : 0, n, xt, rgid);
    const u32 *keys = A.sfx[f] ? rgid : s.g.gid;
    size_t need = 0;
    if (is_max) {
      (void)rocprim::inclusive_scan_by_key(nullptr, need, keys, xt, x, n,
                                           rocprim::maximum<i64>(),
                                           rocprim::equal_to<u32>(),
                                           ctx->stream);
      void *tmp = S.get(need);
      (void)rocprim::inclusive_scan_by_key(tmp, need, keys, xt, x, n,
                                           rocprim::maximum<i64>(),
                                           rocprim::equal_to<u32>(),
                                           ctx->stream);
    } else {
      (void)rocprim::inclusive_scan_by_key(nullptr, need, keys, xt, x, n,
                                           rocprim::minimum<i64>(),
                                           rocprim::equal_to<u32>(),
                                           ctx->stream);
      void *tmp = S.get(need);
      (void)rocprim::inclusive_scan_by_key(tmp, need, keys, xt, x, n,
                                           rocprim::minimum<i64>(),
                                           rocprim::equal_to<u32>(),
                                           ctx->stream);
    }
    A.x[f] = x;
  }
  return A;
}

// Order one eval set of pe->n >= 1 rows as TopK does and derive what the
// emit kernel reads: peer head flags, their max-scan (peer-start rows) and
// their sum-scan (dense ranks). All in scratch.
static WinSnap window_eval(Ctx *ctx, mz_gpu_window *op, mz_gpu_out *pe,
                           WinAggs *aggs) {
  u64 n = pe->n;
  u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  auto &S = (*ctx->scr);
  hipLaunchKernelGGL(k_window_check, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, (const i64 *)pe->diffs, n, op->d_err);
  OrderedSnap s =
      order_snapshot(ctx, kw, vb, op->spec.n_order, op->spec.order, pe);
  WinOrder ord;
  ord.n = op->spec.n_order;
  for (u32 j = 0; j < MZ_GPU_MAX_ORDER; j++) ord.c[j] = op->spec.order[j];
  u32 *flags = (u32 *)S.get(n * 4);
  u32 *hidx = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_window_peer_flags, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, s.keys, kw, s.vals, vb, ord, n, flags,
                     hidx);
  u32 *pstart = (u32 *)S.get(n * 4);
  size_t need = 0;
  (void)rocprim::inclusive_scan(nullptr, need, hidx, pstart, n,
                                rocprim::maximum<u32>(), ctx->stream);
  void *tmp = S.get(need);
  (void)rocprim::inclusive_scan(tmp, need, hidx, pstart, n,
                                rocprim::maximum<u32>(), ctx->stream);
  u32 *pcum = (u32 *)S.get(n * 4);
  inclusive_scan_u32(ctx, flags, pcum, n);
  if (op->has_agg) *aggs = window_agg_prefixes(ctx, op->spec, s, n);
  return WinSnap{s.keys, s.vals, s.pre, s.g.gid, s.g.starts, pstart, pcum, n};
}

int mz_gpu_window_push(mz_gpu_ctx *c, mz_gpu_window *op,
                       const mz_gpu_updates *u, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  const u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  const u32 ovb = op->spec.out.val_bytes;
  const u64 kMaxExpanded = 0x7FFFFFFFull, kMaxTotal = 0xFFFFFFFFull;
  WinFuncs F;
  F.n = op->spec.n_funcs;
  for (u32 f = 0; f < MZ_GPU_MAX_WFUNCS; f++) F.f[f] = op->spec.funcs[f];
  bool negative = false, too_big = false, sum_range = false;
  auto eval = [&](u64 t, mz_gpu_out *oldp, mz_gpu_out *newp, SnapSeg *seg) {
    WinSnap so{}, sn{};
    WinAggs ao{}, an{};
    if (oldp->n) so = window_eval(ctx, op, oldp, &ao);
    if (newp->n) sn = window_eval(ctx, op, newp, &an);
    u64 mo = oldp->n, mn = newp->n;  // output rows of each snapshot
    if (op->expand) {
      // the expanded sizes are read back before anything of that size is
      // allocated, with the error words that say whether they mean
      // anything
      u64 *stage = (u64 *)ctx->pin;
      stage[0] = stage[1] = 0;
      if (so.n)
        HIP_CHECK(hipMemcpyAsync(stage, so.pre + (so.n - 1), 8,
                                 hipMemcpyDeviceToHost, ctx->stream));
      if (sn.n)
        HIP_CHECK(hipMemcpyAsync(stage + 1, sn.pre + (sn.n - 1), 8,
                                 hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(stage + 2, op->d_err, 16,
                               hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      mo = stage[0];
      mn = stage[1];
      negative = stage[2] != 0;
      too_big = stage[3] != 0 || mo > kMaxExpanded || mn > kMaxExpanded;
    }
    if (negative || too_big) return false;
    if (!(mo + mn)) return true;
    seg->cols = flat_alloc(ctx, mo + mn, kw, ovb);
    seg->n = mo + mn;
    const FlatCols &p = seg->cols;
    auto emit = op->has_agg ? k_window_emit<true> : k_window_emit<false>;
    if (mo)
      hipLaunchKernelGGL(emit, dim3(ngrid(mo)), dim3(BLK), 0, ctx->stream, so,
                         F, ao, kw, vb, ovb, op->expand ? 1 : 0, mo, (u64)0,
                         t, (i64)-1, p.keys, p.vals, p.times, p.diffs,
                         op->d_err);
    if (mn)
      hipLaunchKernelGGL(emit, dim3(ngrid(mn)), dim3(BLK), 0, ctx->stream, sn,
                         F, an, kw, vb, ovb, op->expand ? 1 : 0, mn, mo, t,
                         (i64)1, p.keys, p.vals, p.times, p.diffs, op->d_err);
    return true;
  };
  // the error words once everything queued has run: a spec holding SUM
  // needs [1] without expansion too, and [2] is the emit kernels' own
  auto errors = [&](u64 total) -> const char * {
    if (!negative && !too_big) {
      if (total > kMaxTotal) {
        too_big = true;
      } else {
        const u64 *e = (const u64 *)d2h_pinned(ctx, op->d_err, 24);
        negative = e[0] != 0;
        if (op->has_sum) {
          too_big = e[1] != 0;
          sum_range = e[2] != 0;
        }
      }
    }
    if (negative) return "negative multiplicities in window";
    if (too_big) return "window: expanded partition exceeds 2^31 rows";
    if (sum_range) return "window: SUM out of int64 range";
    return nullptr;
  };
  return snapshot_diff_push(c, op->arr, ovb, kMaxTotal, u, eval, errors, out);
}

int mz_gpu_partition(mz_gpu_ctx *c, const mz_gpu_schema *s,
                     const mz_gpu_updates *u, uint32_t nshards,
                     uint64_t *out_keys, uint8_t *out_vals,
                     uint64_t *out_times, int64_t *out_diffs,
                     uint64_t *counts) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  auto &S = (*ctx->scr);
  u32 kw = s->key_words, vb = s->val_bytes;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  u64 n = d.n;
  for (u32 i = 0; i < nshards; i++) counts[i] = 0;
  if (n == 0) return 0;
  u32 *shard = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_shard_of, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     d.keys, kw, n, nshards, shard);
  // stable order by shard: radix sort (shard, perm)
  u32 *perm = (u32 *)S.get(n * 4);
  u32 *perm_out = (u32 *)S.get(n * 4);
  u32 *shard_out = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_iota, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream, perm,
                     n);
  size_t need = 0;
  (void)rocprim::radix_sort_pairs(nullptr, need, shard, shard_out, perm, perm_out,
                            (unsigned)n, 0, 32, ctx->stream);
  void *tmp = S.get(need);
  (void)rocprim::radix_sort_pairs(tmp, need, shard, shard_out, perm, perm_out,
                            (unsigned)n, 0, 32, ctx->stream);
  // gather into caller buffers (device or host staging)
  bool dev_out = u->on_device;
  u64 *gk = dev_out ? out_keys : (u64 *)S.get(n * kw * 8);
  u8 *gv = vb ? (dev_out ? out_vals : (u8 *)S.get(n * vb)) : nullptr;
  u64 *gt = dev_out ? out_times : (u64 *)S.get(n * 8);
  i64 *gd = dev_out ? out_diffs : (i64 *)S.get(n * 8);
  hipLaunchKernelGGL(k_gather_keyrows, dim3(ngrid(n)), dim3(BLK), 0,
                     ctx->stream, d.keys, kw, perm_out, gk, n);
  if (vb)
    hipLaunchKernelGGL(k_gather_valrows, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, d.vals, vb, perm_out, gv, n);
  hipLaunchKernelGGL(k_gather_u64, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     d.times, perm_out, gt, n);
  hipLaunchKernelGGL(k_gather_i64, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     d.diffs, perm_out, gd, n);
  // shard counts on host
  std::vector<u32> hshard(n);
  HIP_CHECK(hipMemcpyAsync(hshard.data(), shard_out, n * 4,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (u64 i = 0; i < n; i++) counts[hshard[i]]++;
  if (!dev_out) {
    HIP_CHECK(hipMemcpy(out_keys, gk, n * kw * 8, hipMemcpyDeviceToHost));
    if (vb) HIP_CHECK(hipMemcpy(out_vals, gv, n * vb, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_times, gt, n * 8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_diffs, gd, n * 8, hipMemcpyDeviceToHost));
  }
  return 0;
}

uint64_t mz_gpu_route_hash(const uint64_t *key_words, uint32_t n_words) {
  return route_hash(key_words, n_words);
}

// ------------------------------------------------------------------ map
// FlatMap/key-preparation analog (render/flat_map.rs; the
// DeltaJoinKeyPreparation map at delta_join.rs:444-464): apply a closure
// (filters + field map) to each update row, no lookup. VAL_STREAM = the
// input val; VAL_LOOKUP is absent.
__global__ void k_map_count(const u64 *keys, u32 kw, const u8 *vals, u32 vb,
                            u64 n, const mz_gpu_closure cl, u32 *flags) {
  GRID_STRIDE(i, n) {
    flags[i] = d_closure_apply(&cl, keys + i * kw,
                               vals ? vals + i * vb : nullptr, nullptr,
                               nullptr, nullptr)
                   ? 1u
                   : 0u;
  }
}

__global__ void k_map_emit(const u64 *keys, u32 kw, const u8 *vals, u32 vb,
                           const u64 *times, const i64 *diffs, u64 n,
                           const mz_gpu_closure cl, const u32 *flags,
                           const u32 *pos, u64 *okeys, u8 *ovals,
                           u64 *otimes, i64 *odiffs) {
  u32 okw = cl.out.key_words, ovb = cl.out.val_bytes;
  GRID_STRIDE(i, n) {
    if (!flags[i]) continue;
    u64 o = pos[i];
    u64 okey[MAX_KW];
    u8 oval[MAX_VB];
    d_closure_apply(&cl, keys + i * kw, vals ? vals + i * vb : nullptr,
                    nullptr, okey, oval);
    for (u32 w = 0; w < okw; w++) okeys[o * okw + w] = okey[w];
    for (u32 c = 0; c < ovb; c++) ovals[o * ovb + c] = oval[c];
    otimes[o] = times[i];
    odiffs[o] = diffs[i];
  }
}

int mz_gpu_map(mz_gpu_ctx *c, const mz_gpu_schema *in,
               const mz_gpu_updates *u, const mz_gpu_closure *cl,
               mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  auto &S = (*ctx->scr);
  u32 kw = in->key_words, vb = in->val_bytes;
  u32 okw = cl->out.key_words, ovb = cl->out.val_bytes;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  u64 n = d.n;
  if (n == 0) {
    *out = empty_out(ctx, okw, ovb);
    return 0;
  }
  u32 *flags = (u32 *)S.get(n * 4);
  hipLaunchKernelGGL(k_map_count, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     d.keys, kw, d.vals, vb, n, *cl, flags);
  u32 *pos = (u32 *)S.get((n + 1) * 4);
  u64 M = exclusive_scan_u32(ctx, flags, pos, n);
  u64 *pk = dnew<u64>(ctx, std::max<u64>(M, 1) * okw);
  u8 *pv = (u8 *)dmalloc(ctx, std::max<u64>(M * ovb, 1));
  u64 *pt = dnew<u64>(ctx, std::max<u64>(M, 1));
  i64 *pd = dnew<i64>(ctx, std::max<u64>(M, 1));
  if (M)
    hipLaunchKernelGGL(k_map_emit, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                       d.keys, kw, d.vals, vb, d.times, d.diffs, n, *cl,
                       flags, pos, pk, pv, pt, pd);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = make_out(pk, pv, pt, pd, M, okw, ovb);
  return 0;
}

// ------------------------------------------------ scalar-expression MFP
// Create-time validation of an expression program (mz_gpu.h lists what is
// refused): the stack discipline by simulation, every COL inside the input
// row, the OUT fields tiling the output row exactly. False with ctx->err
// set when the program is refused.
static bool mfp_validate(Ctx *ctx, const mz_gpu_mfp_spec *sp) {
  auto fail = [&](const std::string &why) {
    ctx->err = "mfp: " + why;
    return false;
  };
  if (sp->n_ops > MZ_GPU_MAX_XOPS)
    return fail("n_ops " + std::to_string(sp->n_ops) + " exceeds " +
                std::to_string(MZ_GPU_MAX_XOPS));
  if (is_varlen(sp->in.val_bytes) || is_varlen(sp->out.val_bytes))
    return fail("varlen schemas unsupported");
  for (const mz_gpu_schema *s : {&sp->in, &sp->out})
    if (s->key_words < 1 || s->key_words > (u32)MAX_KW ||
        s->val_bytes > (u32)MAX_VB)
      return fail("schemas must have 1..2 key words and at most 64 val bytes");
  u32 room[2] = {8 * sp->in.key_words, sp->in.val_bytes};
  u32 oroom[2] = {8 * sp->out.key_words, sp->out.val_bytes};
  u8 written[2][MAX_VB] = {};
  u32 depth = 0;
  for (u32 i = 0; i < sp->n_ops; i++) {
    const mz_gpu_xop &op = sp->ops[i];
    std::string at = "op " + std::to_string(i) + ": ";
    u32 pops, pushes = 1;
    switch (op.op) {
      case MZ_X_COL:
        if (op.src != MZ_SRC_KEY && op.src != MZ_SRC_VAL_STREAM)
          return fail(at + "COL must read MZ_SRC_KEY or MZ_SRC_VAL_STREAM");
        if (op.width != 1 && op.width != 4 && op.width != 8)
          return fail(at + "COL width must be 1, 4 or 8");
        if ((u32)op.off + op.width + (op.nullable ? 1 : 0) > room[op.src])
          return fail(at + "COL reads past the input row's key or val");
        pops = 0;
        break;
      case MZ_X_LIT:
      case MZ_X_NULL: pops = 0; break;
      case MZ_X_NEG:
      case MZ_X_ABS:
      case MZ_X_NOT:
      case MZ_X_IS_NULL: pops = 1; break;
      case MZ_X_IF: pops = 3; break;
      case MZ_X_FILTER:
      case MZ_X_OUT:
        pops = 1;
        pushes = 0;
        break;
      default:
        if (op.op < MZ_X_ADD || op.op > MZ_X_COALESCE)
          return fail(at + "unknown opcode " + std::to_string(op.op));
        pops = 2;
    }
    if (depth < pops) return fail(at + "stack underflow");
    depth = depth - pops + pushes;
    if (depth > MZ_GPU_XSTACK)
      return fail(at + "stack deeper than " + std::to_string(MZ_GPU_XSTACK));
    if (!pushes && depth != 0)
      return fail(at + "stack not empty after the statement");
    if (op.op != MZ_X_OUT) continue;
    if (op.src > 1) return fail(at + "OUT src must be 0 (key) or 1 (val)");
    if (op.width != 1 && op.width != 4 && op.width != 8)
      return fail(at + "OUT width must be 1, 4 or 8");
    if (op.src == 0 && (op.width != 8 || op.nullable))
      return fail(at + "a key OUT is 8 bytes wide and not nullable");
    u32 end = (u32)op.off + op.width + (op.nullable ? 1 : 0);
    if (end > oroom[op.src])
      return fail(at + "OUT writes past the output row's key or val");
    for (u32 b = op.off; b < end; b++) {
      if (written[op.src][b]) return fail(at + "OUT fields overlap");
      written[op.src][b] = 1;
    }
  }
  if (depth != 0) return fail("stack not empty at the end of the program");
  for (u32 s = 0; s < 2; s++)
    for (u32 b = 0; b < oroom[s]; b++)
      if (!written[s][b])
        return fail(std::string("OUT fields leave a gap in the output ") +
                    (s ? "val" : "key"));
  return true;
}

// stage -> k_mfp_eval under the probe protocol's counters and timing
// bracket (run_probe; the queues are exact, so its relaunch never fires)
// -> consolidate (or hand back the raw queue) -> error stream.
int mz_gpu_mfp(mz_gpu_ctx *c, const mz_gpu_mfp_spec *sp,
               const mz_gpu_updates *u, int consolidate, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  if (!mfp_validate(ctx, sp)) return 1;
  (*ctx->scr).reset();
  u32 kw = sp->in.key_words, vb = sp->in.val_bytes;
  u32 okw = sp->out.key_words, ovb = sp->out.val_bytes;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  u64 n = d.n;
  if (n == 0) {
    *out = empty_out(ctx, okw, ovb);
    return 0;
  }
  DeltaView dv{d.keys, d.vals, vb, d.times, d.diffs, n, kw};
  ProbeQueue pq{okw, ovb};
  ProbeCounts r = run_probe(ctx, pq, n, n, 2, n, [&](EmitQueue q) {
    hipLaunchKernelGGL(k_mfp_eval, dim3(ngrid((n + MFP_ROWS - 1) / MFP_ROWS)),
                       dim3(BLK), 0, ctx->stream, dv, *sp, q);
  });
  u64 M = r.M;
  if (ctx->time_kernels)  // run_probe has synced and entered the call
    ctx->probe_alg_bytes +=
        n * (8ull * kw + vb + 16) + M * (8ull * okw + ovb + 16);
  if (!consolidate) {
    // raw rows in queue order; the consumer consolidates
    *out = make_out(pq.q.okeys, pq.q.ovals, pq.q.otimes, pq.q.odiffs, M, okw,
                    ovb);
  } else {
    DevUpdates pin{pq.q.okeys, pq.q.ovals, pq.q.otimes, pq.q.odiffs, M};
    u64 Mc;
    FlatCols o = consolidate_dev(ctx, okw, ovb, pin, &Mc);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    pq.free_ok(ctx);
    *out = make_out(o, Mc, okw, ovb);
  }
  attach_err_stream(ctx, *out, pq, r.E);
  return 0;
}

// ----------------------------------------------- hierarchical min/max op
struct mz_gpu_minmax {
  u32 kw;
  int is_max;
  std::vector<u32> buckets;
  std::vector<mz_gpu_arr> levels;
  std::vector<KeyedTable> states;  // host-counted; capacity fixed at create
};

mz_gpu_minmax *mz_gpu_minmax_create(mz_gpu_ctx *c, const mz_gpu_schema *in,
                                    int is_max, const uint32_t *buckets,
                                    uint32_t n_levels) {
  Ctx *ctx = &c->impl;
  auto *op = new mz_gpu_minmax();
  op->kw = in->key_words;
  op->is_max = is_max;
  op->buckets.assign(buckets, buckets + n_levels);
  op->levels.resize(n_levels);
  op->states.resize(n_levels);
  u32 kw2 = op->kw + 1;
  for (u32 l = 0; l < n_levels; l++) {
    op->levels[l].schema = {kw2, 8};
    // rows [key][exists][value]
    kt_create_at(ctx, op->states[l], kw2, 2, 1ull << 21, nullptr, nullptr);
  }
  return op;
}

// Internal: minmax over already-staged device updates at time t. Does not
// reset the scratch arena (the public entry does) so a caller can keep its
// own staged columns alive across several sub-pushes.
static int minmax_push_dev_impl(Ctx *ctx, mz_gpu_minmax *op, DevUpdates d0,
                                u64 t, mz_gpu_out **out);

int mz_gpu_minmax_push(mz_gpu_ctx *c, mz_gpu_minmax *op,
                       const mz_gpu_updates *u, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  if (u->upper > u->lower + 1) {
    ctx->err = "minmax_push: single-timestamp batches only";
    return -1;
  }
  (*ctx->scr).reset();
  DevUpdates d0 = stage_updates(ctx, u, op->kw, 8);
  return minmax_push_dev_impl(ctx, op, d0, u->lower, out);
}

static int minmax_push_dev_impl(Ctx *ctx, mz_gpu_minmax *op, DevUpdates d0,
                                u64 t, mz_gpu_out **out) {
  auto &S = (*ctx->scr);
  u32 kw = op->kw, kw2 = kw + 1;
  u32 L = (u32)op->buckets.size();
  // level-0 input keys: (key, b0(val))
  u64 n = d0.n;
  u64 *bkeys = (u64 *)S.get(std::max<u64>(n, 1) * kw2 * 8);
  if (n)
    hipLaunchKernelGGL(k_bucket_keys, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, d0.keys, kw, d0.vals, n,
                       op->buckets[0], bkeys);
  DevUpdates cur{bkeys, d0.vals, d0.times, d0.diffs, n};
  // ping-pong correction buffers (owned, freed at the end)
  std::vector<void *> owned;
  u64 *fk = nullptr;
  u8 *fv = nullptr;
  u64 *ft = nullptr;
  i64 *fd = nullptr;
  u64 fM = 0;
  for (u32 l = 0; l < L && cur.n; l++) {
    mz_gpu_arr *A = &op->levels[l];
    DevBatch *nb = arr_insert_dev(ctx, A, cur, t, t + 1);
    u64 G = nb->n_keys;
    if (G == 0) {
      cur.n = 0;
      break;
    }
    // 3-phase state upsert over the changed groups (batch keys = the
    // sorted distinct changed keys), host-counted: the miss total is read
    // back, so the capacity check is exact and fails the push
    KeyedTable &T = op->states[l];
    u32 *gstart = (u32 *)S.get(G * 4);
    hipLaunchKernelGGL(k_iota, dim3(ngrid(G)), dim3(BLK), 0, ctx->stream,
                       gstart, G);
    u32 *found = (u32 *)S.get(G * 4);
    u32 *miss = (u32 *)S.get(G * 4);
    hipLaunchKernelGGL(k_red_lookup, dim3(ngrid(G)), dim3(BLK), 0,
                       ctx->stream, nb->keys, kw2, gstart, G,
                       (const u32 *)nullptr, 0, T.st, found, miss);
    u32 *misspos = (u32 *)S.get((G + 1) * 4);
    u64 Mn = exclusive_scan_u32(ctx, miss, misspos, G);
    if (T.n_rows + Mn > T.st.capacity) {
      for (void *p : owned) dfree(ctx, p);
      ctx->err = "minmax state capacity exceeded";
      return -1;
    }
    if (Mn)
      hipLaunchKernelGGL(k_red_insert, dim3(ngrid(G)), dim3(BLK), 0,
                         ctx->stream, nb->keys, kw2, gstart, G,
                         (const u32 *)nullptr, 0, miss, misspos,
                         T.n_rows, (const u64 *)nullptr, (u64 *)nullptr,
                         T.st);
    // output buffer for this level's corrections
    u32 out_kw = (l + 1 < L) ? kw2 : kw;
    u32 bnext = (l + 1 < L) ? op->buckets[l + 1] : 1;
    u64 cap_out = 2 * G + 16;
    u64 *pk = dnew<u64>(ctx, cap_out * out_kw);
    u8 *pv = (u8 *)dmalloc(ctx, cap_out * 8);
    u64 *pt = dnew<u64>(ctx, cap_out);
    i64 *pd = dnew<i64>(ctx, cap_out);
    owned.insert(owned.end(), {(void *)pk, (void *)pv, (void *)pt,
                               (void *)pd});
    unsigned long long *ocount = (unsigned long long *)S.get(8);
    fill_u64(ctx, (u64 *)ocount, 1, 0);
    BatchList bl;
    bl.n = 0;
    for (auto &b : A->batches)
      if (b.n_upds && bl.n < 12) {
        bl.allpass[bl.n] = 0;
        bl.b[bl.n++] = b;
      }
    hipLaunchKernelGGL(k_minmax_apply, dim3(ngrid(G)), dim3(BLK), 0,
                       ctx->stream, nb->keys, G, kw2, bl, op->is_max,
                       T.st, found, miss, misspos, T.n_rows,
                       out_kw, bnext, t, pk, pv, pt, pd, ocount);
    T.n_rows += Mn;
    unsigned long long M;
    HIP_CHECK(hipMemcpyAsync(&M, ocount, 8, hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    cur = DevUpdates{pk, pv, pt, pd, M};
    if (l + 1 == L) {
      fk = pk;
      fv = pv;
      ft = pt;
      fd = pd;
      fM = M;
    }
  }
  // consolidate the top-level corrections
  u64 Mc = 0;
  DevUpdates fin{fk, fv, ft, fd, fM};
  FlatCols o = consolidate_dev(ctx, kw, 8, fin, &Mc);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (void *p : owned) dfree(ctx, p);
  *out = make_out(o, Mc, kw, 8);
  return 0;
}

void mz_gpu_minmax_drop(mz_gpu_ctx *c, mz_gpu_minmax *op) {
  Ctx *ctx = &c->impl;
  for (auto &lvl : op->levels) {
    for (auto &b : lvl.batches) free_batch(ctx, b);
    lvl.batches.clear();
  }
  for (auto &T : op->states) kt_free(ctx, T);
  delete op;
}

// ------------------------------------------------------ collated reduce op
struct mz_gpu_collation {
  mz_gpu_collation_spec spec;
  CollateLayout L;
  mz_gpu_red *red = nullptr;        // part 0 (null: no accumulable aggs)
  std::vector<mz_gpu_minmax *> mms;  // one part per MIN/MAX aggregate
  std::vector<mz_gpu_aggregate> mm_aggs;
  KeyedTable tbl;  // resident stitch state; d_err[0] capacity,
                   // d_err[1] missing part
  // The parts run on this arena: the main arena holds the staged input
  // and the projected columns across all parts and is reset once per
  // push, while a part may reset its arena freely (a bucket level's spine
  // merge does).
  Scratch sub;
};

namespace {
struct ScrGuard {
  Ctx *c;
  Scratch *prev;
  ScrGuard(Ctx *ctx, Scratch *s) : c(ctx), prev(ctx->scr) {
    s->reset();
    c->scr = s;
  }
  ~ScrGuard() { c->scr = prev; }
};
}  // namespace

static void collation_free(mz_gpu_ctx *c, mz_gpu_collation *op) {
  Ctx *ctx = &c->impl;
  for (mz_gpu_minmax *m : op->mms) mz_gpu_minmax_drop(c, m);
  kt_free(ctx, op->tbl);
  (void)hipStreamSynchronize(ctx->stream);
  op->sub.destroy();
  delete op;
}

mz_gpu_collation *mz_gpu_collation_create(mz_gpu_ctx *c,
                                          const mz_gpu_collation_spec *spec) {
  Ctx *ctx = &c->impl;
  auto fail = [&](const char *msg) -> mz_gpu_collation * {
    ctx->err = msg;
    return nullptr;
  };
  if (is_varlen(spec->in.val_bytes) || is_varlen(spec->out.val_bytes))
    return fail("collation: varlen vals unsupported");
  if (spec->n_aggs < 1 || spec->n_aggs > MZ_GPU_MAX_AGGS)
    return fail("collation: n_aggs out of range");
  u32 kw = spec->in.key_words;
  if (kw < 1 || kw > 2) return fail("collation: key_words must be 1 or 2");
  if (spec->out.key_words != kw || spec->out.val_bytes != 24 * spec->n_aggs)
    return fail("collation: out schema must be (in.key_words, 24 * n_aggs)");
  if (spec->n_levels < 1 || spec->n_levels > 4)
    return fail("collation: n_levels out of range");
  for (u32 l = 0; l < spec->n_levels; l++)
    if (spec->buckets[l] == 0 ||
        (l + 1 == spec->n_levels && spec->buckets[l] != 1))
      return fail("collation: buckets must be non-zero and end with 1");
  u32 n_acc = 0, n_mm = 0;
  for (u32 a = 0; a < spec->n_aggs; a++) {
    const mz_gpu_aggregate &g = spec->aggs[a];
    if (g.func > MZ_AGG_MAX_I64) return fail("collation: unknown aggregate");
    bool mm = g.func >= MZ_AGG_MIN_I64;
    if (mm && g.nullable)
      return fail("collation: nullable MIN/MAX inputs unsupported");
    if (const char *msg = distinct_agg_error(g, spec->in)) {
      ctx->err = std::string("collation: ") + msg;
      return nullptr;
    }
    if (g.func != MZ_AGG_COUNT || g.nullable) {  // COUNT(*) reads nothing
      if (g.width != 4 && g.width != 8)
        return fail("collation: aggregate width must be 4 or 8");
      if ((u64)g.off + g.width + (g.nullable ? 1 : 0) > spec->in.val_bytes)
        return fail("collation: aggregate reads past in.val_bytes");
    }
    (mm ? n_mm : n_acc)++;
  }
  auto *op = new mz_gpu_collation();
  op->spec = *spec;
  // layout: part 0 = accumulable (if any), then the MIN/MAX parts in order
  CollateLayout &L = op->L;
  memset(&L, 0, sizeof(L));
  L.n_aggs = spec->n_aggs;
  u32 part = 0, off = 0;
  mz_gpu_reduce_spec rs{};
  if (n_acc) {
    L.part_off[0] = 0;
    L.part_len[0] = 3 * n_acc;
    off = 3 * n_acc;
    part = 1;
  }
  u32 acc_rank = 0;
  for (u32 a = 0; a < spec->n_aggs; a++) {
    const mz_gpu_aggregate &g = spec->aggs[a];
    if (g.func >= MZ_AGG_MIN_I64) {
      L.part_off[part] = off;
      L.part_len[part] = 1;
      L.slot_src[a] = off;
      L.slot_mm[a] = 1;
      off++;
      part++;
      op->mm_aggs.push_back(g);
    } else {
      L.slot_src[a] = 3 * acc_rank;
      L.slot_mm[a] = 0;
      rs.aggs[acc_rank++] = g;
    }
  }
  L.n_parts = part;
  L.PW = off;
  L.W = n_acc ? 3 * n_acc : 1;
  if (n_acc) {
    rs.n_aggs = n_acc;
    rs.in = spec->in;
    rs.out = {kw, 24 * n_acc};
    op->red = mz_gpu_reduce_create(c, &rs);
    if (!op->red) {
      delete op;
      return nullptr;
    }
  }
  mz_gpu_schema mm_in{kw, 8};
  for (u32 j = 0; j < n_mm; j++)
    op->mms.push_back(mz_gpu_minmax_create(
        c, &mm_in, op->mm_aggs[j].func == MZ_AGG_MAX_I64, spec->buckets,
        spec->n_levels));
  // 1M keys default; grows on demand; env override for tests/tuning
  kt_create(ctx, op->tbl, kw, 1 + L.PW,
            kt_env_cap("MZ_GPU_COL_CAP", 1ull << 20), /*n_err=*/2);
  ctx->cols.push_back(op);
  return op;
}

void mz_gpu_collation_drop(mz_gpu_ctx *c, mz_gpu_collation *op) {
  Ctx *ctx = &c->impl;
  if (op->red) mz_gpu_reduce_drop(c, op->red);
  auto &v = ctx->cols;
  v.erase(std::remove(v.begin(), v.end(), op), v.end());
  collation_free(c, op);
}

int mz_gpu_collation_push(mz_gpu_ctx *c, mz_gpu_collation *op,
                          const mz_gpu_updates *u, mz_gpu_out **out) {
  Ctx *ctx = &c->impl;
  if (u->upper > u->lower + 1) {
    ctx->err = "collation_push: single-timestamp batches only";
    return -1;
  }
  MZ_PROF(ctx, "collation_push");
  // the ONE reset of the main arena: the staged input and the projected
  // columns below must survive every part's push
  (*ctx->scr).reset();
  auto &S = (*ctx->scr);
  const CollateLayout &L = op->L;
  u32 kw = op->spec.in.key_words, vb = op->spec.in.val_bytes;
  u32 ovb = op->spec.out.val_bytes;
  u64 t = u->lower;
  DevUpdates d = stage_updates(ctx, u, kw, vb);
  u64 n = d.n;
  if (n == 0) {
    *out = empty_out(ctx, kw, ovb);
    return 0;
  }
  // ---- parts: each reduction type on its own, over the same input
  std::vector<mz_gpu_out *> pouts(L.n_parts, nullptr);
  auto release_parts = [&]() {
    for (mz_gpu_out *o : pouts)
      if (o) mz_gpu_out_release(c, o);
  };
  u32 part = 0;
  if (op->red) {
    MZ_PROF(ctx, "collation_accumulable");
    ScrGuard sg(ctx, &op->sub);
    if (reduce_push_dev_impl(ctx, op->red, d, u->lower, u->upper,
                             &pouts[0]) != 0)
      return -1;
    part = 1;
  }
  for (size_t j = 0; j < op->mms.size(); j++, part++) {
    MZ_PROF(ctx, "collation_minmax");
    const mz_gpu_aggregate &g = op->mm_aggs[j];
    u8 *pv = (u8 *)S.get(n * 8);
    hipLaunchKernelGGL(k_project_i64, dim3(ngrid(n)), dim3(BLK), 0,
                       ctx->stream, d.vals, vb, (u32)g.off, (u32)g.width, n,
                       pv);
    DevUpdates dp{d.keys, pv, d.times, d.diffs, n};
    ScrGuard sg(ctx, &op->sub);
    if (minmax_push_dev_impl(ctx, op->mms[j], dp, t, &pouts[part]) != 0) {
      release_parts();
      return -1;
    }
  }
  u64 R = 0;
  for (mz_gpu_out *o : pouts) R += o->n;
  if (R == 0) {
    release_parts();
    *out = empty_out(ctx, kw, ovb);
    return 0;
  }
  MZ_PROF(ctx, "collation_stitch");
  // every changed key has a correction row in some part, and an input row
  kt_reserve(ctx, op->tbl, std::min(R, n));
  // ---- tagged stream (key, part, diff, val padded), sorted by key
  u64 *tk = (u64 *)S.get(R * kw * 8);
  u64 *tv = (u64 *)S.get(R * L.W * 8);
  u32 *tp = (u32 *)S.get(R * 4);
  u64 *tt = (u64 *)S.get(R * 8);
  i64 *td = (i64 *)S.get(R * 8);
  u64 base = 0;
  for (u32 p = 0; p < L.n_parts; p++) {
    mz_gpu_out *o = pouts[p];
    if (o->n)
      hipLaunchKernelGGL(k_collate_pack, dim3(ngrid(o->n)), dim3(BLK), 0,
                         ctx->stream, o->keys, o->vals, o->diffs, o->n, kw,
                         L.part_len[p], p, L.W, t, base, tk, tv, tp, tt, td);
    base += o->n;
  }
  u32 *perm = (u32 *)S.get(R * 4);
  sort_updates(ctx, tk, kw, nullptr, 0, tt, R, perm, false);
  u64 *sk = (u64 *)S.get(R * kw * 8);
  hipLaunchKernelGGL(k_gather_keyrows, dim3(ngrid(R)), dim3(BLK), 0,
                     ctx->stream, tk, kw, perm, sk, R);
  // ---- stitch upsert: lookup, insert, apply as three launches
  Groups g = group_sorted(ctx, sk, kw, tt, R);
  Upsert up = kt_upsert(ctx, op->tbl, sk, g, R);
  CorrBuf cb = corr_alloc(ctx, 2 * R + 16, kw, ovb);  // ≤2 rows per key
  hipLaunchKernelGGL(k_collate_apply, dim3(ngrid(R)), dim3(BLK), 0,
                     ctx->stream, sk, kw, perm, tp, td, tv, g.starts, g.gid, R,
                     t, op->tbl.st, up.found, up.miss, up.misspos,
                     op->tbl.d_nrows, L, op->tbl.d_err + 1, cb.pk,
                     (u64 *)cb.pv, cb.pt, cb.pd, cb.ocount);
  kt_commit(ctx, op->tbl, up, g, R);
  // the stitch's one readback: count, table rows, both error words
  const u64 *h = corr_read(ctx, cb, op->tbl.d_nrows, 3);
  u64 emitted = h[0], cap_err = h[2], part_err = h[3];
  op->tbl.n_rows = h[1];
  release_parts();
  if (cap_err || part_err) {
    corr_free(ctx, cb);
    fill_u64(ctx, op->tbl.d_err, 2, 0);
    ctx->err = cap_err ? "collation state capacity exceeded"
                       : "collation: key missing a reduction type";
    return -1;
  }
  *out = corr_finish(ctx, cb, emitted, false);
  return 0;
}

// ---- numeric debug probes (test support; not part of the drop-in surface)
__global__ void k_dbg_f2fp(const double *in, u128 *out, u64 n) {
  GRID_STRIDE(i, n) out[i] = (u128)d_float_to_fixed_point(in[i]);
}
__global__ void k_dbg_i128d(const u128 *in, double *out, u64 n) {
  GRID_STRIDE(i, n) out[i] = i128_to_double((i128)in[i]) / 16777216.0;
}
// xs[n] doubles -> fp_out[2n] u64 (lo,hi of fixed-point encode);
// fp_in[2n] -> dec_out[n] doubles (decode path incl. the /2^24).
void mz_gpu_debug_float_paths(mz_gpu_ctx *c, const double *xs, uint64_t n,
                              uint64_t *fp_out, const uint64_t *fp_in,
                              double *dec_out) {
  Ctx *ctx = &c->impl;
  (*ctx->scr).reset();
  auto &S = (*ctx->scr);
  double *dx = (double *)S.get(n * 8);
  u128 *dfp = (u128 *)S.get(n * 16);
  double *dd = (double *)S.get(n * 8);
  HIP_CHECK(hipMemcpyAsync(dx, xs, n * 8, hipMemcpyHostToDevice,
                           ctx->stream));
  hipLaunchKernelGGL(k_dbg_f2fp, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     dx, dfp, n);
  HIP_CHECK(hipMemcpyAsync(fp_out, dfp, n * 16, hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_CHECK(hipMemcpyAsync(dfp, fp_in, n * 16, hipMemcpyHostToDevice,
                           ctx->stream));
  hipLaunchKernelGGL(k_dbg_i128d, dim3(ngrid(n)), dim3(BLK), 0, ctx->stream,
                     dfp, dd, n);
  HIP_CHECK(hipMemcpyAsync(dec_out, dd, n * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// ---- bench instrumentation (not part of the drop-in surface)
void mz_gpu_set_kernel_timing(mz_gpu_ctx *c, int on) {
  c->impl.time_kernels = on;
}
void mz_gpu_get_probe_stats(mz_gpu_ctx *c, double *ms, uint64_t *rows,
                            uint64_t *launches) {
  *ms = c->impl.probe_ms;
  *rows = c->impl.probe_rows;
  *launches = c->impl.probe_launches;
  c->impl.probe_ms = 0;
  c->impl.probe_rows = 0;
  c->impl.probe_launches = 0;
}
void mz_gpu_get_probe_stats2(mz_gpu_ctx *c, uint64_t *pairs,
                             uint64_t *batches, uint64_t *alg_bytes) {
  *pairs = c->impl.probe_pairs;
  *batches = c->impl.probe_batches;
  *alg_bytes = c->impl.probe_alg_bytes;
  c->impl.probe_pairs = 0;
  c->impl.probe_batches = 0;
  c->impl.probe_alg_bytes = 0;
}

}  // extern "C"
