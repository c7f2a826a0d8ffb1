"""materialize_amd._ffi — ctypes bindings to libmzgpu.so (the product).

Loads the in-tree HIP library. On a machine with a GPU this module FAILS
LOUDLY if the extension is missing or fails to initialize — there is no
CPU fallback on the product path.
"""
import ctypes as C
import os
import subprocess

from ._abi import (Closure, CollationSpec, Finishing, KeyRange, MfpSpec,
                   OutBatch, PeekStats, ReduceSpec, Schema, TemporalSpec,
                   TopKSpec, Updates, WindowSpec, out_to_numpy)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "csrc", "libmzgpu.so")
_LIB = None


class MzGpuError(RuntimeError):
    pass


def _torch_has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def load():
    """Load and bind libmzgpu.so. Raises MzGpuError if unavailable."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        # attempt an in-tree build (hipcc cross-compiles without a GPU)
        try:
            subprocess.run(["make", "-C", os.path.dirname(_LIB_PATH)],
                           check=True, capture_output=True)
        except Exception as e:
            raise MzGpuError(
                f"libmzgpu.so missing at {_LIB_PATH} and in-tree build "
                f"failed: {e}. The HIP extension is required — there is no "
                f"CPU fallback.") from e
    lib = C.CDLL(_LIB_PATH)
    lib.mz_gpu_init.restype = C.c_void_p
    lib.mz_gpu_init.argtypes = [C.c_void_p]
    lib.mz_gpu_fini.argtypes = [C.c_void_p]
    lib.mz_gpu_last_error.restype = C.c_char_p
    lib.mz_gpu_last_error.argtypes = [C.c_void_p]
    lib.mz_gpu_sync.argtypes = [C.c_void_p]
    lib.mz_gpu_arr_create.restype = C.c_void_p
    lib.mz_gpu_arr_create.argtypes = [C.c_void_p, C.POINTER(Schema)]
    lib.mz_gpu_arr_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_arr_push_batch.argtypes = [C.c_void_p, C.c_void_p,
                                          C.POINTER(Updates)]
    lib.mz_gpu_arr_insert.argtypes = [C.c_void_p, C.c_void_p,
                                      C.POINTER(Updates)]
    lib.mz_gpu_arr_set_logical_compaction.argtypes = [C.c_void_p, C.c_void_p,
                                                      C.c_uint64]
    lib.mz_gpu_arr_maintain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.mz_gpu_arr_stats.argtypes = [C.c_void_p, C.c_void_p] + \
        [C.POINTER(C.c_uint64)] * 3
    lib.mz_gpu_out_release.argtypes = [C.c_void_p, C.POINTER(OutBatch)]
    lib.mz_gpu_out_to_host.argtypes = [
        C.c_void_p, C.POINTER(OutBatch), C.POINTER(C.c_uint64),
        C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
    lib.mz_gpu_out_err_to_host.argtypes = [
        C.c_void_p, C.POINTER(OutBatch), C.POINTER(C.c_uint64),
        C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
    lib.mz_gpu_out_voffs_to_host.argtypes = [
        C.c_void_p, C.POINTER(OutBatch), C.POINTER(C.c_uint32)]
    lib.mz_gpu_consolidate.argtypes = [C.c_void_p, C.POINTER(Schema),
                                       C.POINTER(Updates),
                                       C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_join_create.restype = C.c_void_p
    lib.mz_gpu_join_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(Closure)]
    lib.mz_gpu_join_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(Updates),
                                     C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_halfjoin.argtypes = [C.c_void_p, C.c_void_p,
                                    C.POINTER(Updates), C.c_uint32, C.c_int,
                                    C.POINTER(Closure),
                                    C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_halfjoin_raw.argtypes = lib.mz_gpu_halfjoin.argtypes
    lib.mz_gpu_halfjoin2.argtypes = [C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(Closure), C.c_void_p,
                                     C.c_int, C.POINTER(Closure),
                                     C.POINTER(Updates), C.c_uint32,
                                     C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_reduce_create.restype = C.c_void_p
    lib.mz_gpu_reduce_create.argtypes = [C.c_void_p, C.POINTER(ReduceSpec)]
    lib.mz_gpu_reduce_push.argtypes = [C.c_void_p, C.c_void_p,
                                       C.POINTER(Updates),
                                       C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_reduce_push2.argtypes = [C.c_void_p, C.c_void_p,
                                        C.POINTER(Updates),
                                        C.POINTER(Updates),
                                        C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_arr_insert_async.argtypes = [C.c_void_p, C.c_void_p,
                                            C.POINTER(Updates)]
    lib.mz_gpu_arr_flush.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_arr_flush_take.argtypes = [C.c_void_p, C.c_void_p,
                                          C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_prof_dump.argtypes = [C.c_void_p]
    lib.mz_gpu_topk_create.restype = C.c_void_p
    lib.mz_gpu_topk_create.argtypes = [C.c_void_p, C.POINTER(TopKSpec)]
    lib.mz_gpu_topk_push.argtypes = [C.c_void_p, C.c_void_p,
                                     C.POINTER(Updates),
                                     C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_topk_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_threshold_create.restype = C.c_void_p
    lib.mz_gpu_threshold_create.argtypes = [C.c_void_p, C.POINTER(Schema)]
    lib.mz_gpu_threshold_push.argtypes = [C.c_void_p, C.c_void_p,
                                          C.POINTER(Updates),
                                          C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_threshold_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_partition.argtypes = [
        C.c_void_p, C.POINTER(Schema), C.POINTER(Updates), C.c_uint32,
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64),
        C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    lib.mz_gpu_map.argtypes = [C.c_void_p, C.POINTER(Schema),
                               C.POINTER(Updates), C.POINTER(Closure),
                               C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_minmax_create.restype = C.c_void_p
    lib.mz_gpu_minmax_create.argtypes = [C.c_void_p, C.POINTER(Schema),
                                         C.c_int, C.POINTER(C.c_uint32),
                                         C.c_uint32]
    lib.mz_gpu_minmax_push.argtypes = [C.c_void_p, C.c_void_p,
                                       C.POINTER(Updates),
                                       C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_minmax_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_collation_create.restype = C.c_void_p
    lib.mz_gpu_collation_create.argtypes = [C.c_void_p,
                                            C.POINTER(CollationSpec)]
    lib.mz_gpu_collation_push.argtypes = [C.c_void_p, C.c_void_p,
                                          C.POINTER(Updates),
                                          C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_collation_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_join_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_reduce_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_peek.argtypes = [C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_uint64), C.c_uint64,
                                C.c_uint64, C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_peek_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.POINTER(Closure), C.c_int,
                                     C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_peek_select.argtypes = [
        C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(KeyRange),
        C.POINTER(Closure), C.POINTER(Finishing), C.c_int,
        C.POINTER(PeekStats), C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_temporal_create.restype = C.c_void_p
    lib.mz_gpu_temporal_create.argtypes = [C.c_void_p,
                                           C.POINTER(TemporalSpec)]
    lib.mz_gpu_temporal_push.argtypes = [C.c_void_p, C.c_void_p,
                                         C.POINTER(Updates),
                                         C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_temporal_stats.argtypes = [C.c_void_p, C.c_void_p] + \
        [C.POINTER(C.c_uint64)] * 3
    lib.mz_gpu_temporal_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_mfp.argtypes = [C.c_void_p, C.POINTER(MfpSpec),
                               C.POINTER(Updates), C.c_int,
                               C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_window_create.restype = C.c_void_p
    lib.mz_gpu_window_create.argtypes = [C.c_void_p, C.POINTER(WindowSpec)]
    lib.mz_gpu_window_push.argtypes = [C.c_void_p, C.c_void_p,
                                       C.POINTER(Updates),
                                       C.POINTER(C.POINTER(OutBatch))]
    lib.mz_gpu_window_drop.argtypes = [C.c_void_p, C.c_void_p]
    lib.mz_gpu_route_hash.restype = C.c_uint64
    lib.mz_gpu_route_hash.argtypes = [C.POINTER(C.c_uint64), C.c_uint32]
    lib.mz_gpu_set_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    lib.mz_gpu_get_probe_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double),
                                           C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]
    _LIB = lib
    return lib


class GpuCtx:
    """One engine context on one GPU (one driver thread per GPU —
    mirrors a timely worker, server.rs:327-377)."""

    # COUNT/SUM(DISTINCT x) (Aggregate.distinct) is implemented here; the
    # render layer refuses such plans on contexts that do not say so.
    supports_distinct_aggs = True
    # Full-scan peeks (mz_gpu_peek_scan) are implemented here; render_peek
    # refuses contexts that do not say so.
    supports_scan_peek = True
    # Peeks with a key range and an ORDER BY / LIMIT / OFFSET finishing
    # (mz_gpu_peek_select) are implemented here; render_peek refuses plans
    # that need them on contexts that do not say so.
    supports_peek_select = True
    # Temporal filters (mz_gpu_temporal_*) are implemented here;
    # render_temporal_filter refuses contexts that do not say so.
    supports_temporal_filter = True
    # Scalar-expression MFPs (mz_gpu_mfp) are implemented here; render_mfp
    # refuses contexts that do not say so.
    supports_mfp = True
    # Window functions (mz_gpu_window_*) are implemented here; render_window
    # refuses contexts that do not say so.
    supports_window = True

    def __init__(self, device=0):
        self.lib = load()
        from ._abi import Cfg
        cfg = Cfg(hbm_pool_bytes=0, device_index=device)
        self.ctx = self.lib.mz_gpu_init(C.byref(cfg))
        if not self.ctx:
            raise MzGpuError(
                "mz_gpu_init failed: no HIP device available. The product "
                "path requires an MI355X; there is no CPU fallback.")
        # (The round-1 "virgin context" warmup is gone: the fault was
        # hipMemsetAsync fills being lost on a fresh process's first ops —
        # all semantic state init now uses compute-kernel fills in the C
        # layer, so every ABI consumer is covered. DESIGN.md §9.)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.mz_gpu_fini(self.ctx)
            self.ctx = None

    def __del__(self):
        # contexts own multi-GB device state; dropping one without
        # close() must not leak it for the rest of the process
        if os.environ.get("MZ_NO_GCCLOSE"):
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise MzGpuError(self.lib.mz_gpu_last_error(self.ctx).decode())

    def _take(self, outp):
        """Copy an out-batch to host numpy arrays and release it. Any
        error rows (ok/err split) land in self.last_errs as
        (codes, times, diffs)."""
        import numpy as np
        from ._abi import MZ_GPU_VARLEN
        ob = outp.contents
        n = ob.n
        kw, vb = ob.schema.key_words, ob.schema.val_bytes
        keys = np.empty(n * kw, np.uint64)
        if vb == MZ_GPU_VARLEN:
            vals = np.empty(int(ob.val_arena_bytes), np.uint8)
            voffs = np.zeros(n + 1, np.uint32)
            if n:
                self._check(self.lib.mz_gpu_out_voffs_to_host(
                    self.ctx, outp,
                    voffs.ctypes.data_as(C.POINTER(C.c_uint32))))
            self.last_voffs = voffs
        else:
            vals = np.empty(n * vb, np.uint8)
            self.last_voffs = None
        times = np.empty(n, np.uint64)
        diffs = np.empty(n, np.int64)
        if n:
            self._check(self.lib.mz_gpu_out_to_host(
                self.ctx, outp,
                keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                vals.ctypes.data_as(C.POINTER(C.c_uint8)),
                times.ctypes.data_as(C.POINTER(C.c_uint64)),
                diffs.ctypes.data_as(C.POINTER(C.c_int64))))
        en = ob.err_n
        ecodes = np.empty(en, np.uint64)
        etimes = np.empty(en, np.uint64)
        ediffs = np.empty(en, np.int64)
        if en:
            self._check(self.lib.mz_gpu_out_err_to_host(
                self.ctx, outp,
                ecodes.ctypes.data_as(C.POINTER(C.c_uint64)),
                etimes.ctypes.data_as(C.POINTER(C.c_uint64)),
                ediffs.ctypes.data_as(C.POINTER(C.c_int64))))
        self.last_errs = (ecodes, etimes, ediffs)
        self.lib.mz_gpu_out_release(self.ctx, outp)
        return keys.view("int64"), vals, times, diffs

    # --- mirrors of the OracleCtx interface (parity rig symmetry) ---
    def arr_create(self, sch):
        return self.lib.mz_gpu_arr_create(self.ctx, C.byref(sch))

    def arr_push(self, arr, upd):
        self._check(self.lib.mz_gpu_arr_push_batch(self.ctx, arr,
                                                   C.byref(upd)))

    def arr_insert(self, arr, upd):
        """Consolidate raw updates + push, fused (one call)."""
        self._check(self.lib.mz_gpu_arr_insert(self.ctx, arr,
                                               C.byref(upd)))

    def arr_set_logical_compaction(self, arr, frontier):
        self.lib.mz_gpu_arr_set_logical_compaction(self.ctx, arr, frontier)

    def arr_maintain(self, arr, fuel=0):
        self._check(self.lib.mz_gpu_arr_maintain(self.ctx, arr, fuel))

    def arr_stats(self, arr):
        nb, nu, by = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.lib.mz_gpu_arr_stats(self.ctx, arr, C.byref(nb), C.byref(nu),
                                  C.byref(by))
        return nb.value, nu.value, by.value

    def join_create(self, a1, a2, cl):
        return self.lib.mz_gpu_join_create(self.ctx, a1, a2, C.byref(cl))

    def join_push(self, op, side, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_join_push(self.ctx, op, side,
                                              C.byref(upd), C.byref(outp)))
        return self._take(outp)

    def halfjoin(self, lookup, upd, stream_vb, le, cl):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_halfjoin(
            self.ctx, lookup, C.byref(upd), stream_vb, 1 if le else 0,
            C.byref(cl), C.byref(outp)))
        return self._take(outp)

    def reduce_create(self, spec):
        op = self.lib.mz_gpu_reduce_create(self.ctx, C.byref(spec))
        if not op:
            raise MzGpuError(self.lib.mz_gpu_last_error(self.ctx).decode())
        return op

    def reduce_push(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_reduce_push(self.ctx, op, C.byref(upd),
                                                C.byref(outp)))
        return self._take(outp)

    def reduce_drop(self, op):
        """Free the operator, its accumulator table and pair tables."""
        self.lib.mz_gpu_reduce_drop(self.ctx, op)

    def arr_insert_async(self, arr, upd):
        self._check(self.lib.mz_gpu_arr_insert_async(self.ctx, arr,
                                                     C.byref(upd)))

    def arr_flush(self, arr):
        self._check(self.lib.mz_gpu_arr_flush(self.ctx, arr))

    def arr_flush_take(self, arr):
        """Flush, returning the pending insert's consolidated rows as a
        sorted DevOut (None when nothing was pending/empty) — the
        arrangement's update stream (mz_arrange_core's published sealed
        rows, extensions/arrange.rs:69-114)."""
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_arr_flush_take(self.ctx, arr,
                                                   C.byref(outp)))
        if not outp:
            return None
        return self._dev_out(outp, sorted=True)

    def prof_dump(self):
        self.lib.mz_gpu_prof_dump(self.ctx)

    def topk_create(self, spec):
        return self.lib.mz_gpu_topk_create(self.ctx, C.byref(spec))

    def topk_push(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_topk_push(self.ctx, op, C.byref(upd),
                                              C.byref(outp)))
        return self._take(outp)

    def threshold_create(self, sch):
        return self.lib.mz_gpu_threshold_create(self.ctx, C.byref(sch))

    def threshold_push(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_threshold_push(self.ctx, op,
                                                   C.byref(upd),
                                                   C.byref(outp)))
        return self._take(outp)

    def consolidate(self, sch, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_consolidate(self.ctx, C.byref(sch),
                                                C.byref(upd), C.byref(outp)))
        return self._take(outp)

    def route_hash(self, words):
        arr = (C.c_uint64 * len(words))(*[w & 0xFFFFFFFFFFFFFFFF
                                          for w in words])
        return self.lib.mz_gpu_route_hash(arr, len(words))

    def map(self, in_schema, upd, cl):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_map(self.ctx, C.byref(in_schema),
                                        C.byref(upd), C.byref(cl),
                                        C.byref(outp)))
        return self._take(outp)

    def minmax_create(self, in_schema, is_max, buckets):
        arr = (C.c_uint32 * len(buckets))(*buckets)
        return self.lib.mz_gpu_minmax_create(self.ctx, C.byref(in_schema),
                                             1 if is_max else 0, arr,
                                             len(buckets))

    def minmax_push(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_minmax_push(self.ctx, op, C.byref(upd),
                                                C.byref(outp)))
        return self._take(outp)

    def collation_create(self, spec):
        op = self.lib.mz_gpu_collation_create(self.ctx, C.byref(spec))
        if not op:
            raise MzGpuError(self.lib.mz_gpu_last_error(self.ctx).decode())
        return op

    def collation_push(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_collation_push(self.ctx, op,
                                                   C.byref(upd),
                                                   C.byref(outp)))
        return self._take(outp)

    def collation_drop(self, op):
        self.lib.mz_gpu_collation_drop(self.ctx, op)

    def peek(self, arr, keys, time, kw=1):
        """Read (val, summed diff) per requested key as of `time`."""
        import numpy as np
        keys = np.ascontiguousarray(keys, np.int64).ravel()
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_peek(
            self.ctx, arr,
            keys.view(np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)),
            len(keys) // kw, time, C.byref(outp)))
        return self._take(outp)

    def _peek_scan(self, arr, as_of, mfp, allow_negative):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_peek_scan(
            self.ctx, arr, as_of,
            C.byref(mfp) if mfp is not None else None,
            1 if allow_negative else 0, C.byref(outp)))
        return outp

    def peek_scan(self, arr, as_of, mfp=None, allow_negative=False):
        """Read the whole arrangement as of `as_of`: every (key, val) with
        its diffs at t' <= as_of summed, through the closure `mfp` (None =
        identity), consolidated. Host columns like `peek`; rows whose mfp
        evaluation errors land in self.last_errs. A negative net count
        raises MzGpuError unless `allow_negative`."""
        return self._take(self._peek_scan(arr, as_of, mfp, allow_negative))

    def _peek_select(self, arr, as_of, key_range, mfp, finishing,
                     allow_negative):
        outp = C.POINTER(OutBatch)()
        stats = PeekStats()
        ref = lambda x: C.byref(x) if x is not None else None
        self._check(self.lib.mz_gpu_peek_select(
            self.ctx, arr, as_of, ref(key_range), ref(mfp), ref(finishing),
            1 if allow_negative else 0, C.byref(stats), C.byref(outp)))
        self.last_peek_stats = (stats.scanned_vals, stats.rows_matched)
        return outp

    def peek_select(self, arr, as_of, key_range=None, mfp=None,
                    finishing=None, allow_negative=False):
        """peek_scan restricted to the stored keys inside `key_range`
        (abi.key_range) and finished by `finishing` (abi.finishing: ORDER
        BY, OFFSET, LIMIT over the mfp's out rows). Host columns like
        `peek_scan`, in finishing order when there is a finishing; error
        rows land in self.last_errs untouched by the finishing, and
        self.last_peek_stats is (scanned vals, rows before finishing)."""
        return self._take(self._peek_select(arr, as_of, key_range, mfp,
                                            finishing, allow_negative))

    def temporal_create(self, spec):
        op = self.lib.mz_gpu_temporal_create(self.ctx, C.byref(spec))
        if not op:
            raise MzGpuError(self.lib.mz_gpu_last_error(self.ctx).decode())
        return op

    def _temporal_push(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_temporal_push(self.ctx, op,
                                                  C.byref(upd),
                                                  C.byref(outp)))
        return outp

    def temporal_push(self, op, upd):
        """Push a delta with bounds [lower, upper) through a temporal
        filter: host columns of every update below `upper`, from this delta
        and from the held buffer, consolidated; bound errors land in
        self.last_errs. An empty delta is a frontier tick."""
        return self._take(self._temporal_push(op, upd))

    def temporal_stats(self, op):
        """(held rows, smallest held time, frontier); the times are
        2**64 - 1 when nothing is held / before the first push."""
        held, nxt, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.mz_gpu_temporal_stats(
            self.ctx, op, C.byref(held), C.byref(nxt), C.byref(f)))
        return held.value, nxt.value, f.value

    def temporal_drop(self, op):
        self.lib.mz_gpu_temporal_drop(self.ctx, op)

    def _mfp(self, spec, upd, consolidate):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_mfp(self.ctx, C.byref(spec),
                                        C.byref(upd),
                                        1 if consolidate else 0,
                                        C.byref(outp)))
        return outp

    def mfp(self, spec, upd, consolidate=True):
        """Run the expression program `spec` (abi.mfp_spec) over a stream:
        host columns of the passing rows, consolidated and in canonical
        order, or with consolidate=False raw, in queue order. Rows whose
        evaluation errors land in self.last_errs."""
        return self._take(self._mfp(spec, upd, consolidate))

    def window_create(self, spec):
        op = self.lib.mz_gpu_window_create(self.ctx, C.byref(spec))
        if not op:
            raise MzGpuError(self.lib.mz_gpu_last_error(self.ctx).decode())
        return op

    def _window_push(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_window_push(self.ctx, op, C.byref(upd),
                                                C.byref(outp)))
        return outp

    def window_push(self, op, upd):
        """Push a delta through a window-function operator: host columns of
        the corrections (new minus old output rows of every changed
        partition), consolidated and in canonical order. After a failed
        push the operator may only be dropped."""
        return self._take(self._window_push(op, upd))

    def window_drop(self, op):
        self.lib.mz_gpu_window_drop(self.ctx, op)

    # --- device-resident variants (outputs stay on the GPU; used by the
    # render layer to chain stages without host round trips) ---
    def _dev_out(self, outp, sorted=False):
        from .render import DevOut
        return DevOut(self, outp, sorted=sorted)

    def _take_copy(self, outp):
        """Copy an OutBatch to host WITHOUT releasing it."""
        import numpy as np
        ob = outp.contents
        n = ob.n
        kw, vb = ob.schema.key_words, ob.schema.val_bytes
        keys = np.empty(n * kw, np.uint64)
        vals = np.empty(n * vb, np.uint8)
        times = np.empty(n, np.uint64)
        diffs = np.empty(n, np.int64)
        if n:
            self._check(self.lib.mz_gpu_out_to_host(
                self.ctx, outp,
                keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                vals.ctypes.data_as(C.POINTER(C.c_uint8)),
                times.ctypes.data_as(C.POINTER(C.c_uint64)),
                diffs.ctypes.data_as(C.POINTER(C.c_int64))))
        return keys.view("int64"), vals, times, diffs

    def consolidate_dev(self, sch, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_consolidate(self.ctx, C.byref(sch),
                                                C.byref(upd), C.byref(outp)))
        return self._dev_out(outp, sorted=True)

    def peek_scan_dev(self, arr, as_of, mfp=None, allow_negative=False):
        # consolidated output in canonical order
        return self._dev_out(
            self._peek_scan(arr, as_of, mfp, allow_negative), sorted=True)

    def peek_select_dev(self, arr, as_of, key_range=None, mfp=None,
                        finishing=None, allow_negative=False):
        # canonical order only without a finishing
        return self._dev_out(
            self._peek_select(arr, as_of, key_range, mfp, finishing,
                              allow_negative), sorted=finishing is None)

    def temporal_push_dev(self, op, upd):
        # consolidated output in canonical order
        return self._dev_out(self._temporal_push(op, upd), sorted=True)

    def mfp_dev(self, spec, upd, consolidate=True):
        return self._dev_out(self._mfp(spec, upd, consolidate),
                             sorted=bool(consolidate))

    def window_push_dev(self, op, upd):
        # consolidated output in canonical order
        return self._dev_out(self._window_push(op, upd), sorted=True)

    def halfjoin_dev(self, lookup, upd, stream_vb, le, cl):
        # raw (unconsolidated) output: the render layer's consumers —
        # the next probe stage and the reduce — consolidate themselves
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_halfjoin_raw(
            self.ctx, lookup, C.byref(upd), stream_vb, 1 if le else 0,
            C.byref(cl), C.byref(outp)))
        return self._dev_out(outp)

    def halfjoin2_dev(self, lk1, le1, cl1, lk2, le2, cl2, upd, stream_vb):
        # fused two-stage delta path (k_probe_path2); raw output
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_halfjoin2(
            self.ctx, lk1, 1 if le1 else 0, C.byref(cl1), lk2,
            1 if le2 else 0, C.byref(cl2), C.byref(upd), stream_vb,
            C.byref(outp)))
        return self._dev_out(outp)

    def partition_dev(self, sch, upd, nshards, out_tensors):
        """mz_gpu_partition into caller-provided torch device tensors
        (keys, vals-or-None, times, diffs); returns per-shard counts.
        The call synchronizes: the tensors are fully written on return."""
        counts = (C.c_uint64 * nshards)()
        kt, vt, tt, dt = out_tensors
        self._check(self.lib.mz_gpu_partition(
            self.ctx, C.byref(sch), C.byref(upd), nshards,
            C.cast(kt.data_ptr(), C.POINTER(C.c_uint64)),
            (C.cast(vt.data_ptr(), C.POINTER(C.c_uint8))
             if vt is not None else None),
            C.cast(tt.data_ptr(), C.POINTER(C.c_uint64)),
            C.cast(dt.data_ptr(), C.POINTER(C.c_int64)),
            counts))
        return list(counts)

    def join_push_dev(self, op, side, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_join_push(self.ctx, op, side,
                                              C.byref(upd), C.byref(outp)))
        return self._dev_out(outp, sorted=True)  # consolidated output

    def threshold_push_dev(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_threshold_push(self.ctx, op,
                                                   C.byref(upd),
                                                   C.byref(outp)))
        return self._dev_out(outp, sorted=True)  # consolidated output

    def reduce_push_dev(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_reduce_push(self.ctx, op, C.byref(upd),
                                                C.byref(outp)))
        return self._dev_out(outp, sorted=True)  # consolidated output

    def reduce_push2_dev(self, op, u1, u2):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_reduce_push2(
            self.ctx, op, C.byref(u1), C.byref(u2), C.byref(outp)))
        return self._dev_out(outp, sorted=True)  # consolidated output

    def collation_push_dev(self, op, upd):
        outp = C.POINTER(OutBatch)()
        self._check(self.lib.mz_gpu_collation_push(self.ctx, op,
                                                   C.byref(upd),
                                                   C.byref(outp)))
        return self._dev_out(outp, sorted=True)  # consolidated output

    def set_kernel_timing(self, on):
        self.lib.mz_gpu_set_kernel_timing(self.ctx, 1 if on else 0)

    def probe_stats(self):
        ms, rows, launches = C.c_double(), C.c_uint64(), C.c_uint64()
        self.lib.mz_gpu_get_probe_stats(self.ctx, C.byref(ms), C.byref(rows),
                                        C.byref(launches))
        return ms.value, rows.value, launches.value
