"""ctypes mirror of include/mz_gpu.h (the C-ABI drop-in boundary).

These are pure type definitions of the boundary; both the product bindings
(materialize_amd._ffi) and the test-side oracle wrapper (oracle/pyoracle.py)
use them so that parity tests drive both implementations through identical
descriptors.
"""
import ctypes as C

import numpy as np

MZ_SRC_KEY = 0
MZ_SRC_VAL_STREAM = 1
MZ_SRC_VAL_LOOKUP = 2
MZ_SRC_COMPUTE = 3

MZ_CMP_LT, MZ_CMP_LE, MZ_CMP_GT, MZ_CMP_GE, MZ_CMP_EQ, MZ_CMP_NE = range(6)
MZ_COMPUTE_REVENUE = 0
MZ_COMPUTE_CONST0 = 1
MZ_COMPUTE_Q17_QTYLT = 2
MZ_COMPUTE_DIV_I64 = 3
MZ_COMPUTE_MUL_I64 = 4
MZ_COMPUTE_CMP_FIELDS = 5
MZ_GPU_VARLEN = 0xFFFFFFFF
(MZ_AGG_COUNT, MZ_AGG_SUM_I64, MZ_AGG_SUM_F64, MZ_AGG_MIN_I64,
 MZ_AGG_MAX_I64) = range(5)
# hierarchical aggregates (collated reduce only)
AGG_MIN_I64, AGG_MAX_I64 = MZ_AGG_MIN_I64, MZ_AGG_MAX_I64

MZ_GPU_MAX_FILTERS = 6
MZ_GPU_MAX_FIELDS = 8
MZ_GPU_MAX_AGGS = 4

# Finalized aggregate output slot: 24 bytes {u8 null; pad[7]; 16B value}
AGG_SLOT_BYTES = 24


class Schema(C.Structure):
    _fields_ = [("key_words", C.c_uint32), ("val_bytes", C.c_uint32)]


class Updates(C.Structure):
    _fields_ = [
        ("keys", C.POINTER(C.c_uint64)),
        ("vals", C.POINTER(C.c_uint8)),
        ("times", C.POINTER(C.c_uint64)),
        ("diffs", C.POINTER(C.c_int64)),
        ("n", C.c_uint64),
        ("lower", C.c_uint64),
        ("upper", C.c_uint64),
        ("on_device", C.c_int32),
        # sorted=1: rows already in canonical (key, val, time) order (the
        # consolidate output form) -> large-table probes take the
        # streaming merge path instead of hash lookups. 0 always safe.
        ("sorted", C.c_int32),
        # VARLEN schemas: [n+1] offsets into the vals byte arena
        ("val_offs", C.POINTER(C.c_uint32)),
    ]


class Filter(C.Structure):
    _fields_ = [
        ("src", C.c_uint8),
        ("off", C.c_uint16),
        ("width", C.c_uint8),
        ("cmp", C.c_uint8),
        ("imm", C.c_int64),
        ("arg0", C.c_uint16),
        ("arg1", C.c_uint16),
        ("arg0_src", C.c_uint8),
        ("arg1_src", C.c_uint8),
    ]


class Field(C.Structure):
    _fields_ = [
        ("src", C.c_uint8),
        ("off", C.c_uint16),
        ("width", C.c_uint8),
        ("arg0", C.c_uint16),
        ("arg1", C.c_uint16),
        ("arg0_src", C.c_uint8),
        ("arg1_src", C.c_uint8),
    ]


class Closure(C.Structure):
    _fields_ = [
        ("n_filters", C.c_uint32),
        ("filters", Filter * MZ_GPU_MAX_FILTERS),
        ("n_key_fields", C.c_uint32),
        ("key_fields", Field * MZ_GPU_MAX_FIELDS),
        ("n_val_fields", C.c_uint32),
        ("val_fields", Field * MZ_GPU_MAX_FIELDS),
        ("out", Schema),
    ]


class Aggregate(C.Structure):
    _fields_ = [
        ("func", C.c_uint8),
        ("off", C.c_uint16),
        ("width", C.c_uint8),
        ("is_float", C.c_uint8),
        ("nullable", C.c_uint8),
        # COUNT/SUM(DISTINCT x); sits in the struct's former padding byte
        ("distinct", C.c_uint8),
    ]


class ReduceSpec(C.Structure):
    _fields_ = [
        ("n_aggs", C.c_uint32),
        ("aggs", Aggregate * MZ_GPU_MAX_AGGS),
        ("in_", Schema),
        ("out", Schema),
    ]


class CollationSpec(C.Structure):
    """mz_gpu_collation_spec: a GROUP BY mixing COUNT/SUM with MIN/MAX."""
    _fields_ = [
        ("n_aggs", C.c_uint32),
        ("aggs", Aggregate * MZ_GPU_MAX_AGGS),
        ("in_", Schema),
        ("out", Schema),
        ("n_levels", C.c_uint32),
        ("buckets", C.c_uint32 * 4),
    ]


MZ_GPU_MAX_ORDER = 4


class OrderCol(C.Structure):
    _fields_ = [
        ("off", C.c_uint16),
        ("width", C.c_uint8),
        ("desc", C.c_uint8),
    ]


class TopKSpec(C.Structure):
    _fields_ = [
        ("in_", Schema),
        ("offset", C.c_uint64),
        ("limit", C.c_int64),
        ("n_order", C.c_uint32),
        ("order", OrderCol * MZ_GPU_MAX_ORDER),
    ]


MZ_ERR_DIVISION_BY_ZERO = 1
MZ_ERR_TIMESTAMP_OUT_OF_RANGE = 2

# temporal filter (mz_gpu_temporal_*): mz_now() bounds
MZ_TB_LOWER, MZ_TB_UPPER = 0, 1
MZ_GPU_MAX_BOUNDS = 4
MAX_KW, MAX_VB = 2, 64  # widest fixed-width row an operator's kernels hold


class TimeBound(C.Structure):
    """mz_gpu_time_bound: mz_now() >= v (LOWER) or mz_now() < v (UPPER),
    v = the row's datum + add."""
    _fields_ = [
        ("kind", C.c_uint8),
        ("src", C.c_uint8),
        ("off", C.c_uint16),
        ("width", C.c_uint8),
        ("nullable", C.c_uint8),
        ("add", C.c_int64),
    ]


class TemporalSpec(C.Structure):
    """mz_gpu_temporal_spec: an MFP with temporal predicates over one input
    stream."""
    _fields_ = [
        ("in_", Schema),
        ("has_mfp", C.c_int32),
        ("mfp", Closure),
        ("n_bounds", C.c_uint32),
        ("bounds", TimeBound * MZ_GPU_MAX_BOUNDS),
        ("until", C.c_uint64),
        ("initial_rows", C.c_uint64),
    ]


class OutBatch(C.Structure):
    _fields_ = [
        ("keys", C.POINTER(C.c_uint64)),
        ("vals", C.POINTER(C.c_uint8)),
        ("times", C.POINTER(C.c_uint64)),
        ("diffs", C.POINTER(C.c_int64)),
        ("n", C.c_uint64),
        ("on_device", C.c_int32),
        ("schema", Schema),
        # error-row stream (the could_error ok/err split,
        # linear_join.rs:495-541): (code, time, diff) rows
        ("err_n", C.c_uint64),
        ("err_codes", C.POINTER(C.c_uint64)),
        ("err_times", C.POINTER(C.c_uint64)),
        ("err_diffs", C.POINTER(C.c_int64)),
        # VARLEN: [n+1] offsets into vals (the byte arena)
        ("val_offs", C.POINTER(C.c_uint32)),
        ("val_arena_bytes", C.c_uint64),
    ]


class Cfg(C.Structure):
    _fields_ = [("hbm_pool_bytes", C.c_uint64), ("device_index", C.c_uint32)]


def schema(kw, vb):
    return Schema(key_words=kw, val_bytes=vb)


def _as_u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def make_updates(keys, vals, times, diffs, lower, upper, on_device=0,
                 sorted=0, val_offs=None):
    """Build an Updates descriptor over numpy arrays (host memory).

    keys: int64/uint64 array of n*key_words; vals: uint8 array of
    n*val_bytes (or None); times: uint64[n]; diffs: int64[n].
    Keeps references to the arrays on the returned struct (._refs).
    """
    keys = np.ascontiguousarray(keys).view(np.uint64).ravel()
    times = _as_u64(times).ravel()
    diffs = np.ascontiguousarray(diffs, dtype=np.int64).ravel()
    n = len(times)
    u = Updates()
    u.keys = keys.ctypes.data_as(C.POINTER(C.c_uint64))
    if vals is not None and len(vals):
        vals = np.ascontiguousarray(vals, dtype=np.uint8).ravel()
        u.vals = vals.ctypes.data_as(C.POINTER(C.c_uint8))
    else:
        vals = None
        u.vals = None
    u.times = times.ctypes.data_as(C.POINTER(C.c_uint64))
    u.diffs = diffs.ctypes.data_as(C.POINTER(C.c_int64))
    u.n = n
    u.lower = lower
    u.upper = upper
    u.on_device = on_device
    u.sorted = sorted
    if val_offs is not None:
        val_offs = np.ascontiguousarray(val_offs, np.uint32).ravel()
        u.val_offs = val_offs.ctypes.data_as(C.POINTER(C.c_uint32))
    u._refs = (keys, vals, times, diffs, val_offs)
    return u


def make_updates_from_torch(keys_t, vals_t, times_t, diffs_t, lower, upper):
    """Updates descriptor over torch CUDA tensors (on_device=1). Tensors:
    keys int64 [n*kw], vals uint8 [n*vb] or None, times int64 (bit-pattern
    u64) [n], diffs int64 [n]. Keeps tensor refs alive on the struct."""
    u = Updates()
    n = times_t.numel()
    u.keys = C.cast(keys_t.data_ptr(), C.POINTER(C.c_uint64))
    u.vals = (C.cast(vals_t.data_ptr(), C.POINTER(C.c_uint8))
              if vals_t is not None and vals_t.numel() else None)
    u.times = C.cast(times_t.data_ptr(), C.POINTER(C.c_uint64))
    u.diffs = C.cast(diffs_t.data_ptr(), C.POINTER(C.c_int64))
    u.n = n
    u.lower = lower
    u.upper = upper
    u.on_device = 1
    u._refs = (keys_t, vals_t, times_t, diffs_t)
    return u


def out_to_numpy(out, copy=True):
    """Read a host OutBatch into numpy arrays (keys, vals, times, diffs)."""
    n = out.n
    kw = out.schema.key_words
    vb = out.schema.val_bytes
    if n == 0:
        return (np.empty(0, np.int64), np.empty(0, np.uint8),
                np.empty(0, np.uint64), np.empty(0, np.int64))
    keys = np.ctypeslib.as_array(out.keys, shape=(n * kw,)).view(np.int64)
    vals = (np.ctypeslib.as_array(out.vals, shape=(n * vb,))
            if vb else np.empty(0, np.uint8))
    times = np.ctypeslib.as_array(out.times, shape=(n,))
    diffs = np.ctypeslib.as_array(out.diffs, shape=(n,))
    if copy:
        return keys.copy(), vals.copy(), times.copy(), diffs.copy()
    return keys, vals, times, diffs


def filt(src, off, width, cmp, imm, arg0=0, arg1=0, arg0_src=0,
         arg1_src=0):
    return Filter(src=src, off=off, width=width, cmp=cmp, imm=imm,
                  arg0=arg0, arg1=arg1, arg0_src=arg0_src,
                  arg1_src=arg1_src)


def field(src, off, width=8, arg0=0, arg1=0, arg0_src=0, arg1_src=0):
    return Field(src=src, off=off, width=width, arg0=arg0, arg1=arg1,
                 arg0_src=arg0_src, arg1_src=arg1_src)


def closure(filters, key_fields, val_fields, out_schema):
    cl = Closure()
    cl.n_filters = len(filters)
    for i, f in enumerate(filters):
        cl.filters[i] = f
    cl.n_key_fields = len(key_fields)
    for i, f in enumerate(key_fields):
        cl.key_fields[i] = f
    cl.n_val_fields = len(val_fields)
    for i, f in enumerate(val_fields):
        cl.val_fields[i] = f
    cl.out = out_schema
    return cl


def topk_spec(in_schema, order, offset=0, limit=-1):
    """order: list of (off, width, desc) over the val bytes."""
    sp = TopKSpec()
    sp.in_ = in_schema
    sp.offset = offset
    sp.limit = limit
    sp.n_order = len(order)
    for i, (off, width, desc) in enumerate(order):
        sp.order[i] = OrderCol(off=off, width=width, desc=1 if desc else 0)
    return sp


# ------------------------------------------------------------ peek select
# mz_gpu_peek_select: a full-scan peek with a key range and an ORDER BY /
# LIMIT / OFFSET finishing (include/mz_gpu.h states the semantics). The
# rules below are csrc/peek_select_spec.h's, with the same messages.
MZ_KB_UNBOUNDED, MZ_KB_INCLUSIVE, MZ_KB_EXCLUSIVE = range(3)
MZ_GPU_NO_NULL = 0xFFFF


class KeyRange(C.Structure):
    """mz_gpu_key_range: bounds on the stored key, i64-tuple order."""
    _fields_ = [
        ("lo_kind", C.c_uint8),
        ("hi_kind", C.c_uint8),
        ("lo", C.c_int64 * 2),
        ("hi", C.c_int64 * 2),
    ]


class PeekOrder(C.Structure):
    """mz_gpu_peek_order: one ORDER BY column of the peek's out row."""
    _fields_ = [
        ("src", C.c_uint8),
        ("width", C.c_uint8),
        ("desc", C.c_uint8),
        ("nulls_last", C.c_uint8),
        ("off", C.c_uint16),
        ("null_off", C.c_uint16),
    ]


class Finishing(C.Structure):
    """mz_gpu_finishing: RowSetFinishing's order_by, offset and limit."""
    _fields_ = [
        ("n_order", C.c_uint32),
        ("order", PeekOrder * MZ_GPU_MAX_ORDER),
        ("offset", C.c_uint64),
        ("limit", C.c_int64),
    ]


class PeekStats(C.Structure):
    _fields_ = [("scanned_vals", C.c_uint64), ("rows_matched", C.c_uint64)]


def peek_range_error(r, kw):
    """The range rules for an arrangement of kw key words; "" when fine."""
    w = "peek_select: range: "
    if r.lo_kind > MZ_KB_EXCLUSIVE or r.hi_kind > MZ_KB_EXCLUSIVE:
        bad = r.lo_kind if r.lo_kind > MZ_KB_EXCLUSIVE else r.hi_kind
        return w + f"unknown bound kind {bad}"
    for i in range(2):
        if i >= kw and (r.lo[i] or r.hi[i]):
            return w + "nonzero bound word beyond key_words"
        if (r.lo_kind == MZ_KB_UNBOUNDED and r.lo[i]) or \
                (r.hi_kind == MZ_KB_UNBOUNDED and r.hi[i]):
            return w + "nonzero bound word on an unbounded side"
    return ""


def _peek_order_why(oc, okw=None, ovb=None):
    """What is wrong with one order column, as the text that follows
    "order column J"; without an out schema only the rules that need none."""
    if oc.src not in (MZ_SRC_KEY, MZ_SRC_VAL_LOOKUP):
        return ": src must be MZ_SRC_KEY or MZ_SRC_VAL_LOOKUP"
    if oc.src == MZ_SRC_KEY:
        if oc.width != 8:
            return ": a key column must be width 8"
        if oc.off % 8 or (okw is not None and oc.off >= 8 * okw):
            return (": a key column must sit at a word boundary inside the "
                    "out key")
        if oc.null_off != MZ_GPU_NO_NULL:
            return ": a key column takes no null_off"
    else:
        if oc.width not in (4, 8, 16):
            return ": width must be 4, 8 or 16"
        if ovb is not None and oc.off + oc.width > ovb:
            return " reads past the out val"
        if oc.null_off != MZ_GPU_NO_NULL:
            if ovb is not None and oc.null_off >= ovb:
                return ": null_off is past the out val"
            if oc.off <= oc.null_off < oc.off + oc.width:
                return ": null_off is inside its own datum"
    if oc.desc > 1 or oc.nulls_last > 1:
        return ": desc and nulls_last must be 0 or 1"
    return ""


def peek_finishing_error(f, okw, ovb, allow_negative=False):
    """The finishing rules against the out row it orders (okw key words,
    ovb val bytes); "" when fine."""
    p = "peek_select: "
    if f.n_order > MZ_GPU_MAX_ORDER:
        return p + f"n_order must be at most {MZ_GPU_MAX_ORDER}"
    for j in range(f.n_order):
        why = _peek_order_why(f.order[j], okw, ovb)
        if why:
            return p + f"order column {j}" + why
    if allow_negative:
        return p + "a finishing cannot be combined with allow_negative"
    return ""


def key_range(lo=None, hi=None, lo_inclusive=True, hi_inclusive=True, kw=1):
    """Bounds on the stored key: lo / hi are an int (kw == 1) or kw ints,
    None = unbounded on that side."""
    r = KeyRange()

    def side(bound, inclusive, words):
        if bound is None:
            return MZ_KB_UNBOUNDED
        bound = [bound] if np.isscalar(bound) else list(bound)
        if len(bound) != kw:
            raise ValueError(f"peek_select: range: a bound takes {kw} key "
                             f"words, not {len(bound)}")
        for i, x in enumerate(bound):
            words[i] = int(x)
        return MZ_KB_INCLUSIVE if inclusive else MZ_KB_EXCLUSIVE

    if kw not in (1, 2):
        raise ValueError("peek_select: range: key_words must be 1 or 2")
    r.lo_kind = side(lo, lo_inclusive, r.lo)
    r.hi_kind = side(hi, hi_inclusive, r.hi)
    why = peek_range_error(r, kw)
    if why:
        raise ValueError(why)
    return r


def order_by(src, off, width=8, desc=False, nulls_last=None, null_off=None):
    """One ORDER BY column of the peek's out row: MZ_SRC_KEY at byte 8 *
    word, or MZ_SRC_VAL_LOOKUP bytes [off, off + width) as a signed
    little-endian integer. null_off = the val byte that is nonzero when the
    datum is NULL. nulls_last=None is the SQL default: last for ASC, first
    for DESC."""
    if nulls_last is None:
        nulls_last = not desc
    for name, v in (("src", src), ("width", width), ("desc", int(desc)),
                    ("nulls_last", int(nulls_last))):
        if not 0 <= v <= 0xFF:
            raise ValueError(f"peek_select: order column: {name} out of "
                             "range")
    oc = PeekOrder(src=src, width=width, desc=int(desc),
                   nulls_last=int(nulls_last), off=off,
                   null_off=MZ_GPU_NO_NULL if null_off is None else null_off)
    why = _peek_order_why(oc)
    if why:
        raise ValueError("peek_select: order column" + why)
    return oc


def finishing(order=(), limit=None, offset=0):
    """ORDER BY `order` (abi.order_by columns) OFFSET `offset` LIMIT `limit`
    (None = no limit)."""
    order = list(order)
    f = Finishing()
    f.n_order = len(order)
    for j, oc in enumerate(order[:MZ_GPU_MAX_ORDER]):
        f.order[j] = oc
    f.offset = offset
    f.limit = -1 if limit is None else limit
    if f.n_order > MZ_GPU_MAX_ORDER:
        raise ValueError("peek_select: n_order must be at most "
                         f"{MZ_GPU_MAX_ORDER}")
    for j, oc in enumerate(order):
        why = _peek_order_why(oc)
        if why:
            raise ValueError(f"peek_select: order column {j}" + why)
    return f


# ------------------------------------------------------ window functions
# mz_gpu_window_*: ROW_NUMBER, RANK, DENSE_RANK, LAG / LEAD, FIRST_VALUE /
# LAST_VALUE and the aggregates SUM / COUNT / MIN / MAX over a frame, per
# partition (include/mz_gpu.h states the semantics).
(MZ_WF_ROW_NUMBER, MZ_WF_RANK, MZ_WF_DENSE_RANK, MZ_WF_LAG, MZ_WF_LEAD,
 MZ_WF_FIRST_VALUE, MZ_WF_LAST_VALUE) = range(7)
MZ_WF_SUM, MZ_WF_COUNT, MZ_WF_MIN, MZ_WF_MAX = 16, 17, 18, 19  # 7..15 unknown
MZ_WF_FRAME_TO_CURRENT, MZ_WF_FRAME_PARTITION, MZ_WF_FRAME_ROWS = 0, 1, 2
(MZ_WB_UNBOUNDED_PRECEDING, MZ_WB_PRECEDING, MZ_WB_CURRENT_ROW,
 MZ_WB_FOLLOWING, MZ_WB_UNBOUNDED_FOLLOWING) = range(5)
MZ_GPU_MAX_WFUNCS = 4
WF_RANK_SLOT_BYTES = 8    # ROW_NUMBER / RANK / DENSE_RANK / COUNT: an i64
WF_VALUE_SLOT_BYTES = 9   # value functions, SUM / MIN / MAX: i64 + null byte


class _WindowFuncBounds(C.Union):
    _fields_ = [("pad", C.c_uint8), ("bounds", C.c_uint8)]


class _WindowFuncEnd(C.Union):
    _fields_ = [("pad2", C.c_uint32), ("end_offset", C.c_uint32)]


class WindowFunc(C.Structure):
    """mz_gpu_window_func: one window function of a spec. `bounds` and
    `end_offset` (ROWS aggregates) are second names of `pad` and `pad2`."""
    _anonymous_ = ("_bounds", "_end")
    _fields_ = [
        ("func", C.c_uint8),
        ("width", C.c_uint8),
        ("nullable", C.c_uint8),
        ("frame", C.c_uint8),
        ("off", C.c_uint16),
        ("has_default", C.c_uint8),
        ("_bounds", _WindowFuncBounds),
        ("offset", C.c_uint32),
        ("_end", _WindowFuncEnd),
        ("dflt", C.c_int64),
    ]


class WindowSpec(C.Structure):
    """mz_gpu_window_spec: partition schema, ORDER BY and the functions."""
    _fields_ = [
        ("in_", Schema),
        ("n_order", C.c_uint32),
        ("order", OrderCol * MZ_GPU_MAX_ORDER),
        ("n_funcs", C.c_uint32),
        ("funcs", WindowFunc * MZ_GPU_MAX_WFUNCS),
        ("out", Schema),
    ]


def wf_is_agg(func):
    return MZ_WF_SUM <= func <= MZ_WF_MAX


def wf_is_value(func):
    """LAG / LEAD / FIRST_VALUE / LAST_VALUE / SUM / MIN / MAX: the
    functions that fill a 9-byte value slot. COUNT fills an i64."""
    return func >= MZ_WF_LAG and func != MZ_WF_COUNT


def wf_slot_bytes(func):
    return WF_VALUE_SLOT_BYTES if wf_is_value(func) else WF_RANK_SLOT_BYTES


def wf_expands(f):
    """Does the function's value differ between the copies of one row? The
    ranking by position, LAG / LEAD, and a ROWS aggregate unless both ends
    are unbounded (the whole partition)."""
    if wf_is_agg(f.func):
        return f.frame == MZ_WF_FRAME_ROWS and f.bounds != (
            MZ_WB_UNBOUNDED_PRECEDING | MZ_WB_UNBOUNDED_FOLLOWING << 4)
    return f.func in (MZ_WF_ROW_NUMBER, MZ_WF_LAG, MZ_WF_LEAD)


def wf_row_number():
    return WindowFunc(func=MZ_WF_ROW_NUMBER)


def wf_rank():
    return WindowFunc(func=MZ_WF_RANK)


def wf_dense_rank():
    return WindowFunc(func=MZ_WF_DENSE_RANK)


def _wf_lag_lead(func, off, width, k, nullable, default):
    if not 0 <= k < 2**32:
        raise ValueError(f"window: LAG/LEAD offset {k} is not a u32")
    if default is not None and not -2**63 <= default < 2**63:
        raise ValueError(f"window: default {default} is not an i64")
    return WindowFunc(func=func, off=off, width=width,
                      nullable=1 if nullable else 0, offset=k,
                      has_default=0 if default is None else 1,
                      dflt=0 if default is None else default)


def wf_lag(off, width, k=1, nullable=0, default=None):
    """LAG(x, k, default) of the datum at `off`; default None = NULL."""
    return _wf_lag_lead(MZ_WF_LAG, off, width, k, nullable, default)


def wf_lead(off, width, k=1, nullable=0, default=None):
    return _wf_lag_lead(MZ_WF_LEAD, off, width, k, nullable, default)


def wf_first_value(off, width, nullable=0):
    return WindowFunc(func=MZ_WF_FIRST_VALUE, off=off, width=width,
                      nullable=1 if nullable else 0)


def wf_last_value(off, width, nullable=0, frame=MZ_WF_FRAME_TO_CURRENT):
    return WindowFunc(func=MZ_WF_LAST_VALUE, off=off, width=width,
                      nullable=1 if nullable else 0, frame=frame)


UNBOUNDED_PRECEDING = (MZ_WB_UNBOUNDED_PRECEDING, 0)
CURRENT_ROW = (MZ_WB_CURRENT_ROW, 0)
UNBOUNDED_FOLLOWING = (MZ_WB_UNBOUNDED_FOLLOWING, 0)


def preceding(k):
    return (MZ_WB_PRECEDING, k)


def following(k):
    return (MZ_WB_FOLLOWING, k)


def _wf_agg(func, off, width, nullable, frame, start, end):
    """One aggregate. `start` / `end` are (MZ_WB_* kind, k) pairs — the
    names above — and either of them selects MZ_WF_FRAME_ROWS; with neither,
    `frame` (default: the SQL default, MZ_WF_FRAME_TO_CURRENT) stands."""
    f = WindowFunc(func=func, off=off, width=width,
                   nullable=1 if nullable else 0)
    if start is None and end is None:
        f.frame = MZ_WF_FRAME_TO_CURRENT if frame is None else frame
        return f
    if frame not in (None, MZ_WF_FRAME_ROWS):
        raise ValueError("window: start / end bounds need MZ_WF_FRAME_ROWS")
    (sk, k), (ek, k2) = (start or UNBOUNDED_PRECEDING), (end or CURRENT_ROW)
    for kind, n in ((sk, k), (ek, k2)):
        if not 0 <= kind < 16:
            raise ValueError(f"window: bound kind {kind} is not a nibble")
        if not 0 <= n < 2**32:
            raise ValueError(f"window: frame offset {n} is not a u32")
    f.frame = MZ_WF_FRAME_ROWS
    f.bounds = sk | ek << 4
    f.offset, f.end_offset = k, k2
    return f


def wf_sum(off, width, nullable=0, frame=None, start=None, end=None):
    """SUM(x) OVER the frame, of the datum at `off`. abi.wf_sum(8, 8,
    start=abi.preceding(2), end=abi.CURRENT_ROW) is ROWS BETWEEN 2 PRECEDING
    AND CURRENT ROW; a missing start is UNBOUNDED PRECEDING, a missing end
    CURRENT ROW."""
    return _wf_agg(MZ_WF_SUM, off, width, nullable, frame, start, end)


def wf_count(off=0, width=0, nullable=0, frame=None, start=None, end=None):
    """COUNT(x) OVER the frame; width 0 (the default) is COUNT(*)."""
    return _wf_agg(MZ_WF_COUNT, off, width, nullable, frame, start, end)


def wf_min(off, width, nullable=0, frame=None, start=None, end=None):
    return _wf_agg(MZ_WF_MIN, off, width, nullable, frame, start, end)


def wf_max(off, width, nullable=0, frame=None, start=None, end=None):
    return _wf_agg(MZ_WF_MAX, off, width, nullable, frame, start, end)


def _window_agg_check(who, f, vb):
    """An aggregate's create-time rules, as window_agg_error in
    csrc/window_spec.h."""
    if f.frame > MZ_WF_FRAME_ROWS:
        raise ValueError(f"{who}: unknown frame {f.frame}")
    star = f.func == MZ_WF_COUNT and f.width == 0
    if not star and f.width not in (4, 8):
        raise ValueError(f"{who}: datum width must be 4 or 8"
                         + (", or 0 for COUNT(*)" if f.func == MZ_WF_COUNT
                            else ""))
    if star and (f.off or f.nullable):
        raise ValueError(f"{who}: COUNT(*) takes no datum")
    if not star and f.off + f.width + (1 if f.nullable else 0) > vb:
        raise ValueError(f"{who} reads past in.val_bytes ({vb})")
    if f.has_default or f.dflt:
        raise ValueError(f"{who}: an aggregate takes no default")
    if f.frame != MZ_WF_FRAME_ROWS:
        if f.bounds or f.offset or f.end_offset:
            raise ValueError(f"{who}: bounds and offsets need "
                             "MZ_WF_FRAME_ROWS")
        return
    sk, ek = f.bounds & 15, f.bounds >> 4
    PREC, FOLL = MZ_WB_PRECEDING, MZ_WB_FOLLOWING
    for kind in (sk, ek):
        if kind > MZ_WB_UNBOUNDED_FOLLOWING:
            raise ValueError(f"{who}: unknown bound kind {kind}")
    if sk == MZ_WB_UNBOUNDED_FOLLOWING:
        raise ValueError(f"{who}: a frame cannot start at UNBOUNDED "
                         "FOLLOWING")
    if ek == MZ_WB_UNBOUNDED_PRECEDING:
        raise ValueError(f"{who}: a frame cannot end at UNBOUNDED PRECEDING")
    if sk == MZ_WB_CURRENT_ROW and ek == PREC:
        raise ValueError(f"{who}: a frame starting at CURRENT ROW cannot "
                         "end PRECEDING")
    if sk == FOLL and ek in (PREC, MZ_WB_CURRENT_ROW):
        raise ValueError(f"{who}: a frame starting FOLLOWING cannot end "
                         "PRECEDING or at CURRENT ROW")
    if (f.offset and sk not in (PREC, FOLL)) or \
            (f.end_offset and ek not in (PREC, FOLL)):
        raise ValueError(f"{who}: an offset on an UNBOUNDED or CURRENT ROW "
                         "bound")
    if f.func in (MZ_WF_MIN, MZ_WF_MAX) and \
            sk != MZ_WB_UNBOUNDED_PRECEDING and \
            ek != MZ_WB_UNBOUNDED_FOLLOWING:
        raise ValueError(f"{who}: MIN / MAX over a ROWS frame bounded on "
                         "both sides is not provided (it needs a "
                         "range-minimum structure)")


def window_spec(in_schema, order, funcs, out=None):
    """mz_gpu_window_spec over rows of `in_schema`: `order` a list of
    (off, width, desc) over the val bytes (may be empty), `funcs` 1..4 wf_*
    items. Derives `out` (in val ++ one slot per function; a caller's `out`
    must be that schema) and checks the operator's create-time rules here
    as well as in the C layer (ValueError)."""
    order, funcs = list(order), list(funcs)
    kw, vb = in_schema.key_words, in_schema.val_bytes
    if vb == MZ_GPU_VARLEN:
        raise ValueError("window: varlen vals unsupported")
    if not 1 <= kw <= MAX_KW:
        raise ValueError("window: key_words must be 1 or 2")
    if not 1 <= len(funcs) <= MZ_GPU_MAX_WFUNCS:
        raise ValueError(f"window: n_funcs must be 1..{MZ_GPU_MAX_WFUNCS}, "
                         f"got {len(funcs)}")
    if len(order) > MZ_GPU_MAX_ORDER:
        raise ValueError(f"window: n_order must be at most "
                         f"{MZ_GPU_MAX_ORDER}, got {len(order)}")
    for j, (off, width, _) in enumerate(order):
        if width not in (4, 8):
            raise ValueError(f"window: order column {j}: width must be 4 "
                             "or 8")
        if off + width > vb:
            raise ValueError(f"window: order column {j} reads past "
                             f"in.val_bytes ({vb})")
    ovb = vb
    for i, f in enumerate(funcs):
        if wf_is_agg(f.func):
            _window_agg_check(f"window: func {i}", f, vb)
            ovb += wf_slot_bytes(f.func)
            continue
        if f.func > MZ_WF_LAST_VALUE:
            raise ValueError(f"window: func {i}: unknown func {f.func}")
        # MZ_WF_FRAME_ROWS is the aggregates' alone
        if f.frame > MZ_WF_FRAME_ROWS or (
                f.frame > MZ_WF_FRAME_PARTITION
                and f.func == MZ_WF_LAST_VALUE):
            raise ValueError(f"window: func {i}: unknown frame {f.frame}")
        if f.frame and f.func != MZ_WF_LAST_VALUE:
            raise ValueError(f"window: func {i}: a frame is for LAST_VALUE "
                             "only")
        if wf_is_value(f.func):
            if f.width not in (4, 8):
                raise ValueError(f"window: func {i}: datum width must be 4 "
                                 "or 8")
            if f.off + f.width + (1 if f.nullable else 0) > vb:
                raise ValueError(f"window: func {i} reads past in.val_bytes "
                                 f"({vb})")
        ovb += wf_slot_bytes(f.func)
    if ovb > MAX_VB:
        raise ValueError(f"window: out val is {ovb} bytes, more than "
                         f"{MAX_VB}")
    if out is not None and (out.key_words, out.val_bytes) != (kw, ovb):
        raise ValueError(f"window: out schema must be {kw} key words and "
                         f"{ovb} val bytes (in val ++ slots)")
    sp = WindowSpec()
    sp.in_ = in_schema
    sp.n_order = len(order)
    for j, (off, width, desc) in enumerate(order):
        sp.order[j] = OrderCol(off=off, width=width, desc=1 if desc else 0)
    sp.n_funcs = len(funcs)
    for i, f in enumerate(funcs):
        sp.funcs[i] = f
    sp.out = Schema(key_words=kw, val_bytes=ovb)
    return sp


def is_distinct(agg):
    """COUNT/SUM(DISTINCT x). MIN/MAX carry the flag without effect: the
    extremum of a set is that of the multiset."""
    return bool(agg.distinct) and agg.func in (MZ_AGG_COUNT, MZ_AGG_SUM_I64,
                                               MZ_AGG_SUM_F64)


def _check_distinct(who, i, a, in_schema):
    """The create-time rules for a distinct aggregate (mz_gpu.h), checked
    here as well as in the C layer (ValueError)."""
    if not is_distinct(a):
        return
    if a.func == MZ_AGG_SUM_F64 or a.is_float:
        raise ValueError(f"{who}: aggregate {i}: DISTINCT over a float "
                         "datum is unsupported")
    if a.width not in (4, 8):
        raise ValueError(f"{who}: aggregate {i}: DISTINCT datum width must "
                         "be 4 or 8")
    if a.off + a.width + (1 if a.nullable else 0) > in_schema.val_bytes:
        raise ValueError(f"{who}: aggregate {i}: DISTINCT datum reads past "
                         f"in.val_bytes ({in_schema.val_bytes})")


def reduce_spec(aggs, in_schema):
    sp = ReduceSpec()
    sp.n_aggs = len(aggs)
    for i, a in enumerate(aggs):
        _check_distinct("reduce", i, a, in_schema)
        sp.aggs[i] = a
    sp.in_ = in_schema
    sp.out = Schema(key_words=in_schema.key_words,
                    val_bytes=AGG_SLOT_BYTES * len(aggs))
    return sp


def is_hierarchical(agg):
    """MIN/MAX: maintained by the bucket tree, not by accumulation."""
    return agg.func in (MZ_AGG_MIN_I64, MZ_AGG_MAX_I64)


def collation_spec(aggs, in_schema, buckets=(256, 16, 1)):
    """mz_gpu_collation_spec for `aggs` (SQL order, any mix of the five
    funcs) over `in_schema`. Fills `out` and checks the operator's
    restrictions here as well as in the C layer (ValueError)."""
    aggs = list(aggs)
    buckets = list(buckets)
    if not 1 <= len(aggs) <= MZ_GPU_MAX_AGGS:
        raise ValueError(
            f"collation: n_aggs must be 1..{MZ_GPU_MAX_AGGS}, "
            f"got {len(aggs)}")
    if in_schema.val_bytes == MZ_GPU_VARLEN:
        raise ValueError("collation: varlen vals unsupported")
    if in_schema.key_words not in (1, 2):
        raise ValueError("collation: key_words must be 1 or 2")
    if not 1 <= len(buckets) <= 4:
        raise ValueError("collation: 1..4 bucket levels")
    if any(b < 1 for b in buckets) or buckets[-1] != 1:
        raise ValueError("collation: buckets must be positive and end "
                         "with 1")
    for i, a in enumerate(aggs):
        if a.func > MZ_AGG_MAX_I64:
            raise ValueError(f"collation: aggregate {i}: unknown func "
                             f"{a.func}")
        if is_hierarchical(a) and a.nullable:
            raise ValueError(f"collation: aggregate {i}: nullable MIN/MAX "
                             "inputs unsupported")
        _check_distinct("collation", i, a, in_schema)
        if a.func == MZ_AGG_COUNT and not a.nullable:
            continue  # COUNT(*) reads nothing
        if a.width not in (4, 8):
            raise ValueError(f"collation: aggregate {i}: width must be 4 "
                             "or 8")
        if a.off + a.width + (1 if a.nullable else 0) > in_schema.val_bytes:
            raise ValueError(f"collation: aggregate {i} reads past "
                             f"in.val_bytes ({in_schema.val_bytes})")
    sp = CollationSpec()
    sp.n_aggs = len(aggs)
    for i, a in enumerate(aggs):
        sp.aggs[i] = a
    sp.in_ = in_schema
    sp.out = Schema(key_words=in_schema.key_words,
                    val_bytes=AGG_SLOT_BYTES * len(aggs))
    sp.n_levels = len(buckets)
    for i, b in enumerate(buckets):
        sp.buckets[i] = b
    return sp


def collation_parts(spec):
    """The operator's part order for `spec`: part 0 is the accumulable
    sub-reduce (the indices of its aggregates, in their relative order;
    absent when there are none), then one part per MIN/MAX aggregate.
    Returns a list of index lists into spec.aggs."""
    idx = range(spec.n_aggs)
    acc = [i for i in idx if not is_hierarchical(spec.aggs[i])]
    parts = [acc] if acc else []
    parts += [[i] for i in idx if is_hierarchical(spec.aggs[i])]
    return parts


def time_bound(cmp, src, off, width=8, add=0, nullable=0):
    """The bounds of the SQL predicate `mz_now() <cmp> datum + add`, as a
    list — the lowering of MfpPlan::create_from (src/expr/src/linear.rs),
    which steps `<=` and `>` forward by one to reach the two canonical
    forms `mz_now() >= v` (LOWER) and `mz_now() < v` (UPPER). `=` is both;
    `<>` is not a temporal predicate (ValueError, as the reference rejects
    it)."""
    def b(kind, a):
        if not -2**63 <= a < 2**63:
            raise ValueError(f"temporal: bound offset {a} is not an i64")
        return TimeBound(kind=kind, src=src, off=off, width=width,
                         nullable=1 if nullable else 0, add=a)
    if cmp == MZ_CMP_GE:
        return [b(MZ_TB_LOWER, add)]
    if cmp == MZ_CMP_GT:
        return [b(MZ_TB_LOWER, add + 1)]
    if cmp == MZ_CMP_LT:
        return [b(MZ_TB_UPPER, add)]
    if cmp == MZ_CMP_LE:
        return [b(MZ_TB_UPPER, add + 1)]
    if cmp == MZ_CMP_EQ:
        return [b(MZ_TB_LOWER, add), b(MZ_TB_UPPER, add + 1)]
    raise ValueError("temporal: mz_now() <> expr is not a temporal "
                     f"predicate (comparator {cmp})")


def _closure_reads(cl):
    """(src, off, bytes) of every read a closure makes of its inputs, and
    its fields as (field, is_val) pairs."""
    reads = []
    for f in cl.filters[:cl.n_filters]:
        w = 4 if f.width == 4 else 8
        if f.src != MZ_SRC_COMPUTE:
            reads.append((f.src, f.off, w))
        elif f.off == MZ_COMPUTE_Q17_QTYLT:
            reads += [(f.arg0_src, f.arg0, 8), (f.arg1_src, f.arg1, 32)]
        elif f.off == MZ_COMPUTE_CMP_FIELDS:
            reads += [(f.arg0_src, f.arg0, w), (f.arg1_src, f.arg1, w)]
    for f in (list(cl.key_fields[:cl.n_key_fields])
              + list(cl.val_fields[:cl.n_val_fields])):
        if f.src != MZ_SRC_COMPUTE:
            reads.append((f.src, f.off, f.width))
        elif f.off != MZ_COMPUTE_CONST0:
            reads += [(f.arg0_src, f.arg0, 8), (f.arg1_src, f.arg1, 8)]
    return reads


def temporal_spec(in_schema, bounds, mfp=None, until=None, initial_rows=0):
    """mz_gpu_temporal_spec for the temporal predicates `bounds` (TimeBound
    items or the lists time_bound returns, in evaluation order) over rows of
    `in_schema`, with the non-temporal filters and the projection in `mfp`
    (a closure over MZ_SRC_KEY / MZ_SRC_VAL_STREAM; None = the row as it
    is). `until` drops outputs at or beyond it (None = no limit). Checks the
    operator's create-time restrictions here as well as in the C layer
    (ValueError)."""
    flat = []
    for b in bounds:
        flat += list(b) if isinstance(b, (list, tuple)) else [b]
    kw, vb = in_schema.key_words, in_schema.val_bytes
    if vb == MZ_GPU_VARLEN:
        raise ValueError("temporal: varlen vals unsupported")
    if not 1 <= kw <= MAX_KW or vb > MAX_VB:
        raise ValueError("temporal: in schema must have 1..2 key words and "
                         "at most 64 val bytes")
    if not 1 <= len(flat) <= MZ_GPU_MAX_BOUNDS:
        raise ValueError(f"temporal: n_bounds must be 1..{MZ_GPU_MAX_BOUNDS}"
                         f", got {len(flat)}")

    def room(src):
        return 8 * kw if src == MZ_SRC_KEY else vb

    for i, b in enumerate(flat):
        if b.kind not in (MZ_TB_LOWER, MZ_TB_UPPER):
            raise ValueError(f"temporal: bound {i}: unknown kind {b.kind}")
        if b.src not in (MZ_SRC_KEY, MZ_SRC_VAL_STREAM):
            raise ValueError(f"temporal: bound {i} must read MZ_SRC_KEY or "
                             "MZ_SRC_VAL_STREAM")
        if b.width not in (4, 8):
            raise ValueError(f"temporal: bound {i}: width must be 4 or 8")
        if b.off + b.width + (1 if b.nullable else 0) > room(b.src):
            raise ValueError(f"temporal: bound {i} reads past the input "
                             "row's key or val (offset out of range)")
    if mfp is not None:
        for src, off, nbytes in _closure_reads(mfp):
            if src == MZ_SRC_VAL_LOOKUP:
                raise ValueError("temporal: mfp reads MZ_SRC_VAL_LOOKUP; a "
                                 "temporal filter has no lookup side")
            if src not in (MZ_SRC_KEY, MZ_SRC_VAL_STREAM):
                raise ValueError(f"temporal: mfp reads unknown source {src}")
            if off + nbytes > room(src):
                raise ValueError("temporal: mfp reads past the input row's "
                                 "key or val (offset out of range)")
        for fields, want, what in (
                (mfp.key_fields[:mfp.n_key_fields], 8 * mfp.out.key_words,
                 "key"),
                (mfp.val_fields[:mfp.n_val_fields], mfp.out.val_bytes,
                 "val")):
            width = 0
            for f in fields:
                if f.src == MZ_SRC_COMPUTE and f.off == MZ_COMPUTE_DIV_I64:
                    raise ValueError(
                        "temporal: the projection may not contain a field "
                        "that can error (MZ_COMPUTE_DIV_I64); put the "
                        "division in a following map")
                width += 8 if f.src == MZ_SRC_COMPUTE else f.width
            if width != want:
                raise ValueError(f"temporal: mfp {what} fields are {width} "
                                 f"bytes wide, its out schema says {want}")
        if not 1 <= mfp.out.key_words <= MAX_KW \
                or mfp.out.val_bytes > MAX_VB:
            raise ValueError("temporal: mfp out schema wider than 2 key "
                             "words / 64 val bytes")
    sp = TemporalSpec()
    sp.in_ = in_schema
    sp.has_mfp = 0 if mfp is None else 1
    if mfp is not None:
        sp.mfp = mfp
    sp.n_bounds = len(flat)
    for i, b in enumerate(flat):
        sp.bounds[i] = b
    sp.until = 0xFFFFFFFFFFFFFFFF if until is None else until
    sp.initial_rows = initial_rows
    return sp


# ------------------------------------------------- scalar-expression MFP
# mz_gpu_mfp: a postfix expression program over one update stream
# (include/mz_gpu.h states the semantics).
(MZ_X_COL, MZ_X_LIT, MZ_X_NULL, MZ_X_NEG, MZ_X_ABS, MZ_X_NOT, MZ_X_IS_NULL,
 MZ_X_ADD, MZ_X_SUB, MZ_X_MUL, MZ_X_DIV, MZ_X_MOD, MZ_X_LT, MZ_X_LE, MZ_X_GT,
 MZ_X_GE, MZ_X_EQ, MZ_X_NE, MZ_X_AND, MZ_X_OR, MZ_X_COALESCE, MZ_X_IF,
 MZ_X_FILTER, MZ_X_OUT) = range(24)
MZ_ERR_INT64_OUT_OF_RANGE = 3
MZ_ERR_NUMERIC_FIELD_OVERFLOW = 4
MZ_ERR_INT32_OUT_OF_RANGE = 5
MZ_ERR_UNEXPECTED_NULL = 6
MZ_GPU_MAX_XOPS = 64
MZ_GPU_XSTACK = 8


class XOp(C.Structure):
    """mz_gpu_xop: one postfix instruction."""
    _fields_ = [
        ("op", C.c_uint8),
        ("src", C.c_uint8),
        ("width", C.c_uint8),
        ("nullable", C.c_uint8),
        ("off", C.c_uint16),
        ("pad", C.c_uint16),
        ("imm", C.c_int64),
    ]


class MfpSpec(C.Structure):
    """mz_gpu_mfp_spec: the program and the schemas it maps between."""
    _fields_ = [
        ("n_ops", C.c_uint32),
        ("ops", XOp * MZ_GPU_MAX_XOPS),
        ("in_", Schema),
        ("out", Schema),
    ]


_X_ARITH = (MZ_X_ADD, MZ_X_SUB, MZ_X_MUL, MZ_X_DIV, MZ_X_MOD)
_X_CMP = (MZ_X_LT, MZ_X_LE, MZ_X_GT, MZ_X_GE, MZ_X_EQ, MZ_X_NE)


class Expr:
    """A scalar expression tree with a type, "int" or "bool". Leaves come
    from x_col / x_lit / x_null; Python operators and x_abs / x_is_null /
    x_if / x_coalesce build the rest and check operand types (ValueError).
    `==` and `!=` build comparisons, so trees are compared by identity."""

    def __init__(self, op, typ, args=(), src=0, off=0, width=0, nullable=0,
                 imm=0):
        self.op, self.typ, self.args = op, typ, tuple(args)
        self.src, self.off, self.width = src, off, width
        self.nullable, self.imm = nullable, imm

    __hash__ = object.__hash__

    def _bin(self, op, other, swap=False):
        a, b = x_expr(self), x_expr(other)
        if swap:
            a, b = b, a
        if op in (MZ_X_AND, MZ_X_OR):
            want, typ = "bool", "bool"
        else:
            want, typ = "int", ("int" if op in _X_ARITH else "bool")
        for e in (a, b):
            if e.typ != want:
                raise ValueError(f"mfp: operator {op} takes {want} operands, "
                                 f"got {e.typ}")
        return Expr(op, typ, (a, b))

    def __add__(self, o): return self._bin(MZ_X_ADD, o)
    def __radd__(self, o): return self._bin(MZ_X_ADD, o, True)
    def __sub__(self, o): return self._bin(MZ_X_SUB, o)
    def __rsub__(self, o): return self._bin(MZ_X_SUB, o, True)
    def __mul__(self, o): return self._bin(MZ_X_MUL, o)
    def __rmul__(self, o): return self._bin(MZ_X_MUL, o, True)
    def __floordiv__(self, o): return self._bin(MZ_X_DIV, o)
    def __rfloordiv__(self, o): return self._bin(MZ_X_DIV, o, True)
    def __mod__(self, o): return self._bin(MZ_X_MOD, o)
    def __rmod__(self, o): return self._bin(MZ_X_MOD, o, True)
    def __lt__(self, o): return self._bin(MZ_X_LT, o)
    def __le__(self, o): return self._bin(MZ_X_LE, o)
    def __gt__(self, o): return self._bin(MZ_X_GT, o)
    def __ge__(self, o): return self._bin(MZ_X_GE, o)
    def __eq__(self, o): return self._bin(MZ_X_EQ, o)
    def __ne__(self, o): return self._bin(MZ_X_NE, o)
    def __and__(self, o): return self._bin(MZ_X_AND, o)
    def __rand__(self, o): return self._bin(MZ_X_AND, o, True)
    def __or__(self, o): return self._bin(MZ_X_OR, o)
    def __ror__(self, o): return self._bin(MZ_X_OR, o, True)

    def _un(self, op, want, typ):
        if want is not None and self.typ != want:
            raise ValueError(f"mfp: operator {op} takes a {want} operand, "
                             f"got {self.typ}")
        return Expr(op, typ, (self,))

    def __neg__(self): return self._un(MZ_X_NEG, "int", "int")
    def __invert__(self): return self._un(MZ_X_NOT, "bool", "bool")

    def __bool__(self):
        raise TypeError("an mfp Expr has no truth value; use & | ~")


def x_expr(v):
    """An Expr as it is; a Python bool or int as a literal."""
    return v if isinstance(v, Expr) else x_lit(v)


def x_col(src, off, width=8, nullable=0):
    """The input row's datum at (src, off): a 4- or 8-byte signed LE integer,
    or (width 1) a boolean byte; `nullable` = a null byte follows it."""
    if width not in (1, 4, 8):
        raise ValueError("mfp: column width must be 1, 4 or 8")
    return Expr(MZ_X_COL, "bool" if width == 1 else "int", src=src, off=off,
                width=width, nullable=1 if nullable else 0)


def x_lit(v):
    if isinstance(v, (bool, np.bool_)):
        return Expr(MZ_X_LIT, "bool", imm=int(v))
    v = int(v)
    if not -2**63 <= v < 2**63:
        raise ValueError(f"mfp: literal {v} is not an i64")
    return Expr(MZ_X_LIT, "int", imm=v)


def x_null(typ):
    if typ not in ("int", "bool"):
        raise ValueError(f"mfp: unknown type {typ!r}")
    return Expr(MZ_X_NULL, typ)


def x_abs(e):
    return x_expr(e)._un(MZ_X_ABS, "int", "int")


def x_is_null(e):
    return x_expr(e)._un(MZ_X_IS_NULL, None, "bool")


def x_if(cond, then, els):
    cond, then, els = x_expr(cond), x_expr(then), x_expr(els)
    if cond.typ != "bool":
        raise ValueError("mfp: the IF condition must be bool")
    if then.typ != els.typ:
        raise ValueError("mfp: the IF branches differ in type")
    return Expr(MZ_X_IF, then.typ, (cond, then, els))


def x_coalesce(first, *rest):
    """COALESCE(first, *rest), right-nested."""
    es = [x_expr(first)] + [x_expr(r) for r in rest]
    if any(e.typ != es[0].typ for e in es):
        raise ValueError("mfp: the COALESCE arguments differ in type")
    acc = es[-1]
    for e in reversed(es[:-1]):
        acc = Expr(MZ_X_COALESCE, e.typ, (e, acc))
    return acc


class XStmt:
    """FILTER or OUT: a statement of an mfp program."""

    def __init__(self, op, expr, src=0, off=0, width=0, nullable=0):
        self.op, self.expr = op, x_expr(expr)
        self.src, self.off, self.width = src, off, width
        self.nullable = 1 if nullable else 0


def x_filter(e):
    return XStmt(MZ_X_FILTER, e)


def x_out_key(e, off):
    return XStmt(MZ_X_OUT, e, src=0, off=off, width=8)


def x_out_val(e, off, width, nullable=0):
    return XStmt(MZ_X_OUT, e, src=1, off=off, width=width, nullable=nullable)


def _x_emit(e, ops):
    """Postfix: operands left to right, then the operator."""
    for a in e.args:
        _x_emit(a, ops)
    ops.append(XOp(op=e.op, src=e.src, width=e.width, nullable=e.nullable,
                   off=e.off, imm=e.imm))


def mfp_spec(in_schema, out_schema, statements):
    """mz_gpu_mfp_spec for `statements` (x_filter / x_out_key / x_out_val
    items, run in the given order) over rows of `in_schema`, producing rows
    of `out_schema`. Checks the statements' types and every create-time rule
    of the C layer (ValueError)."""
    for s in (in_schema, out_schema):
        if s.val_bytes == MZ_GPU_VARLEN:
            raise ValueError("mfp: varlen schemas unsupported")
        if not 1 <= s.key_words <= MAX_KW or s.val_bytes > MAX_VB:
            raise ValueError("mfp: schemas must have 1..2 key words and at "
                             "most 64 val bytes")
    ops = []
    for i, st in enumerate(statements):
        if st.op == MZ_X_FILTER:
            if st.expr.typ != "bool":
                raise ValueError(f"mfp: statement {i}: FILTER takes a bool")
        else:
            if st.width not in (1, 4, 8):
                raise ValueError(f"mfp: statement {i}: OUT width must be 1, "
                                 "4 or 8")
            if (st.width == 1) != (st.expr.typ == "bool"):
                raise ValueError(f"mfp: statement {i}: width 1 is for bool "
                                 "values and only for them")
            if st.src == 0 and (st.width != 8 or st.nullable):
                raise ValueError(f"mfp: statement {i}: a key OUT is 8 bytes "
                                 "wide and not nullable")
        _x_emit(st.expr, ops)
        ops.append(XOp(op=st.op, src=st.src, width=st.width,
                       nullable=st.nullable, off=st.off))
    if len(ops) > MZ_GPU_MAX_XOPS:
        raise ValueError(f"mfp: the program has {len(ops)} ops, more than "
                         f"{MZ_GPU_MAX_XOPS}")
    room = (8 * in_schema.key_words, in_schema.val_bytes)
    oroom = (8 * out_schema.key_words, out_schema.val_bytes)
    written = ([0] * oroom[0], [0] * oroom[1])
    arity = {MZ_X_COL: 0, MZ_X_LIT: 0, MZ_X_NULL: 0, MZ_X_NEG: 1,
             MZ_X_ABS: 1, MZ_X_NOT: 1, MZ_X_IS_NULL: 1, MZ_X_IF: 3,
             MZ_X_FILTER: 1, MZ_X_OUT: 1}
    depth = 0
    for i, op in enumerate(ops):
        if op.op == MZ_X_COL:
            if op.src not in (MZ_SRC_KEY, MZ_SRC_VAL_STREAM):
                raise ValueError(f"mfp: op {i}: COL must read MZ_SRC_KEY or "
                                 "MZ_SRC_VAL_STREAM")
            if op.off + op.width + op.nullable > room[op.src]:
                raise ValueError(f"mfp: op {i}: COL reads past the input "
                                 "row's key or val")
        depth -= arity.get(op.op, 2)
        assert depth >= 0  # trees cannot underflow
        if op.op in (MZ_X_FILTER, MZ_X_OUT):
            assert depth == 0
        else:
            depth += 1
        if depth > MZ_GPU_XSTACK:
            raise ValueError(f"mfp: op {i}: the expression needs a stack "
                             f"deeper than {MZ_GPU_XSTACK}")
        if op.op != MZ_X_OUT:
            continue
        end = op.off + op.width + op.nullable
        if end > oroom[op.src]:
            raise ValueError(f"mfp: op {i}: OUT writes past the output "
                             "row's key or val")
        for b in range(op.off, end):
            if written[op.src][b]:
                raise ValueError(f"mfp: op {i}: OUT fields overlap")
            written[op.src][b] = 1
    for s, what in ((0, "key"), (1, "val")):
        if not all(written[s]):
            raise ValueError(f"mfp: OUT fields leave a gap in the output "
                             f"{what}")
    sp = MfpSpec()
    sp.n_ops = len(ops)
    for i, op in enumerate(ops):
        sp.ops[i] = op
    sp.in_ = in_schema
    sp.out = out_schema
    return sp
