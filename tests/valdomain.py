"""Shared helpers for the value-domain and hash-wraparound tests.

Three things live here, none of them a test:

* the independent reference: rows as Python tuples (keys as signed ints,
  vals as the canonical tuple of zero-padded little-endian u64 words, time
  as an int) consolidated by naive.consolidate;
* input generators that plant the exact extremes of every column and a
  small model of the sort planner's chunking, so each case can assert the
  planner shape it is meant to hit. The model describes INPUTS (which
  chunks the planner has to form for them); it is never an oracle for
  outputs;
* a host-side search for keys whose splitmix64 route hash lands in the
  last slots of every small power-of-two table.
"""
import numpy as np

import naive

I64_MIN, I64_MAX = -2**63, 2**63 - 1
U64_MAX = 2**64 - 1
M64 = 2**64

# the engine's composite-key limits (materialize_amd/csrc/mzgpu.hip)
MAX_COMP = 6
CHUNK_BITS = 64


def canon_val_key(vb_bytes):
    """The engine's canonical val order: zero-padded LE u64 words,
    unsigned ascending (oracle.cpp cmp_val)."""
    b = bytes(vb_bytes)
    words = []
    for off in range(0, len(b), 8):
        chunk = b[off:off + 8] + bytes(8 - min(8, len(b) - off))
        words.append(int.from_bytes(chunk, "little"))
    return tuple(words)


def wrap_i64(d):
    return ((d + 2**63) % 2**64) - 2**63


# ------------------------------------------------------------- references

def to_rows(keys, vals, times, diffs, kw, vb):
    """Columns (any of the layouts the contexts take or return) -> list of
    (key tuple, canonical val tuple, time, diff) Python rows. For a fixed
    vb the canonical tuple is injective in the val bytes, so equal rows
    mean equal bytes."""
    times = np.asarray(times).astype(np.uint64).ravel()
    n = len(times)
    keys = np.asarray(keys).ravel().view(np.int64).reshape(n, kw)
    vals = (np.asarray(vals, np.uint8).reshape(n, vb) if vb
            else np.zeros((n, 0), np.uint8))
    diffs = np.asarray(diffs).ravel().view(np.int64)
    return [(tuple(int(x) for x in keys[i]), canon_val_key(vals[i]),
             int(times[i]), int(diffs[i])) for i in range(n)]


def naive_consolidated(batch, kw, vb):
    return naive.consolidate(to_rows(*batch, kw, vb))


def naive_as_of(batches, as_of, kw, vb):
    """What a whole-arrangement read as of `as_of` returns: every update
    at t <= as_of, its time advanced to as_of, consolidated."""
    rows = []
    for b in batches:
        rows += [(k, v, as_of, d) for k, v, t, d in to_rows(*b, kw, vb)
                 if t <= as_of]
    return naive.consolidate(rows)


def deciding_columns(rows):
    """Over sorted rows: (varying columns, columns that decide the order
    of some neighbouring pair, i.e. the first column the pair differs
    in). Columns are numbered over the flattened (key words, val words,
    time). A column that varies but never decides is one whose order a
    wrong sort could get away with."""
    flat = [k + v + (t,) for k, v, t, _ in rows]
    varying = {c for c in range(len(flat[0]))
               if len({r[c] for r in flat}) > 1} if flat else set()
    deciding = set()
    for a, b in zip(flat, flat[1:]):
        deciding.add(next(c for c in range(len(a)) if a[c] != b[c]))
    return varying, deciding


def updates(abi, batch, lower, upper):
    keys, vals, times, diffs = batch
    return abi.make_updates(keys.ravel(),
                            vals.ravel() if vals.shape[1] else None,
                            times, diffs, lower, upper)


def assert_cols_equal(got, want, what):
    for a, b, col in zip(got, want, ("keys", "vals", "times", "diffs")):
        a = np.ascontiguousarray(np.asarray(a)).view(np.uint8)
        b = np.ascontiguousarray(np.asarray(b)).view(np.uint8)
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {col}")


# ---------------------------------------------------------- planner model

def column_spans(batch, kw, vb, time_major=False):
    """Per sort column (lo, hi) of the planner's unsigned sort keys, in
    LSD order: time, val words high to low, key words high to low (or,
    time-major: key words high to low, then time)."""
    keys, vals, times, _ = batch
    n = len(times)
    tcol = [int(x) for x in np.asarray(times, np.uint64)]
    vcols = []
    if not time_major:
        words = [canon_val_key(vals[i]) for i in range(n)] if vb else []
        for w in reversed(range((vb + 7) // 8)):
            vcols.append([r[w] for r in words])
    kcols = []
    for w in reversed(range(kw)):
        kcols.append([(int(x) + 2**63) % M64 for x in keys[:, w]])
    cols = kcols + [tcol] if time_major else [tcol] + vcols + kcols
    return [(min(c), max(c)) for c in cols]


def pad_spans(spans):
    """The bounds a cached plan is primed with: one eighth of the span
    (plus one) on each side of every non-constant column, saturating."""
    out = []
    for lo, hi in spans:
        if lo < hi:
            pad = (hi - lo) // 8 + 1
            lo, hi = lo - min(pad, lo), min(hi + pad, U64_MAX)
        out.append((lo, hi))
    return out


def covered(cached, spans):
    """Does a cached plan cover a batch with these exact spans."""
    return all((lo >= clo and hi <= chi) or (clo == chi and lo == hi)
               for (clo, chi), (lo, hi) in zip(cached, spans))


def chunk_bits(spans):
    """Composite chunks the planner forms for these spans: a list of
    chunks, each the list of its columns' live bit counts in LSD order.
    Constant columns take no pass; a chunk holds at most 64 bits and at
    most MAX_COMP columns."""
    chunks = []
    cur = 0
    for lo, hi in spans:
        if hi <= lo:
            continue
        bits = (hi - lo).bit_length()
        if not chunks or cur + bits > CHUNK_BITS or \
                len(chunks[-1]) == MAX_COMP:
            chunks.append([])
            cur = 0
        chunks[-1].append(bits)
        cur += bits
    return chunks


def plan_shape(batch, kw, vb, time_major=False):
    return chunk_bits(column_spans(batch, kw, vb, time_major))


# -------------------------------------------------------------- generators
#
# A generator fills n rows; rows 0 and 1 carry the planted extremes of
# every column and are never overwritten. _mix then rewrites some of the
# other rows in place into copies of their neighbours: exact duplicates
# whose diffs cancel, duplicates whose diffs add (some with extreme diffs,
# so the i64 sum wraps), and copies that differ from their original in one
# sort column only: one key word, one val word, or the time. Random wide
# rows never tie on their leading columns, so without these copies the
# order of every column but the most significant would go unchecked.
# Every value _mix writes already occurs in the same column, so the column
# spans, and with them the planner shape, are unchanged.

EDGE_DIFFS = np.array([I64_MIN, I64_MAX, 2**62, -1, 1], np.int64)


def _mix(rng, batch):
    keys, vals, times, diffs = batch
    n = len(times)
    if n < 8:
        return batch
    idx = 2 + rng.permutation(n - 2)
    g = len(idx) // 12
    src = idx[4 * g:5 * g]
    donor = idx[5 * g:6 * g]

    def copy_rows(dst, src=src):
        keys[dst], vals[dst], times[dst] = keys[src], vals[src], times[src]

    gone = idx[6 * g:7 * g]                   # cancelling duplicates
    diffs[gone[:g // 2]] = rng.choice(EDGE_DIFFS, g // 2)
    copy_rows(idx[0:g], gone)
    diffs[idx[0:g]] = (-diffs[gone].view(np.uint64)).view(np.int64)
    copy_rows(idx[g:2 * g])                   # adding duplicates, wrapping
    diffs[idx[g:2 * g]] = rng.choice(EDGE_DIFFS, g)
    kw = keys.shape[1]
    for w in range(kw):                       # differ in one key word only
        dst = idx[(2 + w) * g:(3 + w) * g]
        copy_rows(dst)
        keys[dst, w] = keys[donor, w]
    dst = idx[7 * g:8 * g]                    # differ in the time only
    copy_rows(dst)
    times[dst] = times[donor]
    nwords = (vals.shape[1] + 7) // 8
    for r in range(8, 11 if nwords else 8):   # differ in one val word only
        dst = idx[r * g:(r + 1) * g]
        copy_rows(dst)
        for d, s, w in zip(dst, donor, rng.integers(0, nwords, g)):
            vals[d, 8 * w:8 * w + 8] = vals[s, 8 * w:8 * w + 8]
    return batch


def _diffs(rng, n):
    return rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.int64), n)


def _u64(rng, n):
    return rng.integers(0, 2**64, n, dtype=np.uint64)


def gen_full(rng, n, kw, vb):
    """Every column full width: each key word holds INT64_MIN and
    INT64_MAX, each val byte 0x00 and 0xFF, time 0 and 2^64 - 1."""
    keys = _u64(rng, n * kw).view(np.int64).reshape(n, kw)
    vals = rng.integers(0, 256, (n, vb), dtype=np.uint8)
    times = _u64(rng, n)
    keys[0], vals[0], times[0] = I64_MIN, 0x00, 0
    if n > 1:
        keys[1], vals[1], times[1] = I64_MAX, 0xFF, U64_MAX
    return _mix(rng, (keys, vals, times, _diffs(rng, n)))


def _ranged(rng, n, lo, span):
    """n u64 values in [lo, lo + span], both ends planted in rows 0, 1."""
    x = lo + rng.integers(0, span + 1, n, dtype=np.uint64)
    x[0], x[1] = lo, lo + span
    return x.astype(np.uint64)


def gen_spans(rng, n, tspan, vspan, kspan):
    """kw = 1, vb = 8 with exact spans (0 = constant) on time, the val
    word and the key; every column sits at an offset, so the subtracted
    minimum matters."""
    times = _ranged(rng, n, 2**63 - 5, tspan)
    vword = _ranged(rng, n, 0xA5000000FFFFFFF0, vspan)
    kflip = _ranged(rng, n, 2**63 - 2**31 + 7, kspan)  # straddles zero
    keys = (kflip ^ np.uint64(2**63)).view(np.int64).reshape(n, 1)
    vals = vword.view(np.uint8).reshape(n, 8).copy()
    return _mix(rng, (keys, vals, times, _diffs(rng, n)))


def gen_narrow(rng, n, kw, vb):
    """Every column 2-3 live bits wide: keys -3..4, the low byte of each
    val word 0..5 under constant high bytes (some >= 0x80), times 0..4
    above 2^63."""
    keys = rng.integers(-3, 5, (n, kw)).astype(np.int64)
    vals = np.tile((0x81 + 7 * np.arange(vb)).astype(np.uint8), (n, 1))
    vals[:, 0::8] = rng.integers(0, 6, (n, (vb + 7) // 8), dtype=np.uint8)
    times = np.uint64(2**63) + rng.integers(0, 5, n, dtype=np.uint64)
    keys[0], vals[0, 0::8], times[0] = -3, 0, 2**63
    keys[1], vals[1, 0::8], times[1] = 4, 5, 2**63 + 4
    return _mix(rng, (keys, vals, times, _diffs(rng, n)))


def gen_const_mixed(rng, n):
    """kw = 2, vb = 16: key word 0 constant at INT64_MIN and val word 1
    constant at all-0xFF bytes beside full-width neighbours."""
    keys, vals, times, diffs = gen_full(rng, n, 2, 16)
    keys[:, 0] = I64_MIN
    vals[:, 8:] = 0xFF
    return keys, vals, times, diffs


def gen_all_const(rng, n):
    """n identical rows (kw = 2, vb = 12): no column takes a pass."""
    keys = np.tile(np.array([I64_MIN, I64_MAX], np.int64), (n, 1))
    vals = np.tile(np.array([0x80, 0xFF, 0, 0x7F] * 3, np.uint8), (n, 1))
    times = np.full(n, 2**63, np.uint64)
    return keys, vals, times, _diffs(rng, n) + 4  # positive: sum != 0


PARTIAL_BYTES = np.array([0x00, 0x7F, 0x80, 0xFF], np.uint8)


def gen_partial(rng, n, vb):
    """kw = 1; val bytes from {0x00, 0x7F, 0x80, 0xFF}, so the order
    inside the partial last word is decided by its high bytes alone. The
    full words before it take one of three patterns, so many rows tie on
    them and are ordered by the partial word."""
    keys = rng.integers(0, 8, (n, 1)).astype(np.int64)
    vals = rng.choice(PARTIAL_BYTES, (n, vb))
    lead = np.array([[0x00] * 8, [0xFF] * 8, [0x80, 0x7F] * 4], np.uint8)
    for w in range(vb // 8):
        vals[:, 8 * w:8 * w + 8] = lead[rng.integers(0, 3, n)]
    times = rng.integers(0, 4, n).astype(np.uint64)
    keys[0], vals[0], times[0] = 0, 0x00, 0
    keys[1], vals[1], times[1] = 7, 0xFF, 3
    return _mix(rng, (keys, vals, times, _diffs(rng, n)))


SIGN_KEYS = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX],
                     np.int64)


def gen_sign(rng, n, kw):
    """Keys on both sides of the sign-bit flip; vb = 8 vals 0..7, times
    0..3."""
    keys = rng.choice(SIGN_KEYS, (n, kw))
    vals = np.zeros((n, 8), np.uint8)
    vals[:, 0] = rng.integers(0, 8, n)
    times = rng.integers(0, 4, n).astype(np.uint64)
    keys[0], vals[0, 0], times[0] = I64_MIN, 0, 0
    keys[1], vals[1, 0], times[1] = I64_MAX, 7, 3
    return _mix(rng, (keys, vals, times, _diffs(rng, n)))


EDGE_KEYS = np.array([I64_MIN, I64_MAX, -1, 0, 1], np.int64)
EDGE_BYTES = np.array([0, 1, 127, 128, 255], np.uint8)
EDGE_TIMES = np.array([0, 1, 2**63 - 1, 2**63, U64_MAX], np.uint64)
EDGE_GRID = [(2, 16), (1, 12), (1, 1), (2, 80), (1, 0)]


def gen_edges(rng, n, kw, vb):
    """Nothing but edge values in every column, diffs included."""
    return (rng.choice(EDGE_KEYS, (n, kw)), rng.choice(EDGE_BYTES, (n, vb)),
            rng.choice(EDGE_TIMES, n), rng.choice(EDGE_DIFFS, n))


F = [64]  # a full-width column is a chunk of its own

# name -> (kw, vb, generator(rng), expected planner shape)
CONSOLIDATE_CASES = {
    # 1. all columns full width: odd (5, 3) and even (4) chunk counts
    "full_kw2_vb16": (2, 16, lambda r: gen_full(r, 1500, 2, 16), [F] * 5),
    "full_kw1_vb8": (1, 8, lambda r: gen_full(r, 1500, 1, 8), [F] * 3),
    "full_kw2_vb8": (2, 8, lambda r: gen_full(r, 1500, 2, 8), [F] * 4),
    # 2. packing that lands exactly on 64 bits, and just past it
    "bits_32_32": (1, 8, lambda r: gen_spans(r, 1200, 0, 2**32 - 1,
                                             2**32 - 1), [[32, 32]]),
    "bits_33_32": (1, 8, lambda r: gen_spans(r, 1200, 0, 2**33 - 1,
                                             2**32 - 1), [[33], [32]]),
    "bits_32_32_5": (1, 8, lambda r: gen_spans(r, 1200, 2**31, 2**31, 31),
                     [[32, 32], [5]]),
    # 3. the 6-column limit
    "cols_7": (1, 40, lambda r: gen_narrow(r, 1200, 1, 40), None),
    "cols_8": (2, 40, lambda r: gen_narrow(r, 1200, 2, 40), None),
    "cols_13": (2, 80, lambda r: gen_narrow(r, 1200, 2, 80), None),
    # 4. constant columns beside wide ones; nothing but constants
    "const_mixed": (2, 16, lambda r: gen_const_mixed(r, 1500), [F] * 3),
    "const_all": (2, 12, lambda r: gen_all_const(r, 700), []),
    "const_one_row": (2, 12, lambda r: gen_all_const(r, 1), []),
    # 5. partial last val word
    "partial_vb1": (1, 1, lambda r: gen_partial(r, 1000, 1), [[2, 8, 3]]),
    "partial_vb9": (1, 9, lambda r: gen_partial(r, 1000, 9),
                    [[2, 8], F, [3]]),
    "partial_vb12": (1, 12, lambda r: gen_partial(r, 1000, 12),
                     [[2, 32], F, [3]]),
    "partial_vb15": (1, 15, lambda r: gen_partial(r, 1000, 15),
                     [[2, 56], F, [3]]),
    # 6. the sign boundary
    "sign_kw1": (1, 8, lambda r: gen_sign(r, 1000, 1), [[2, 3], F]),
    "sign_kw2": (2, 8, lambda r: gen_sign(r, 1000, 2), [[2, 3], F, F]),
    # 7. wave and block tails of case 1
    "tail_1": (2, 16, lambda r: gen_full(r, 1, 2, 16), []),
    "tail_63": (2, 16, lambda r: gen_full(r, 63, 2, 16), [F] * 5),
    "tail_64": (2, 16, lambda r: gen_full(r, 64, 2, 16), [F] * 5),
    "tail_65": (2, 16, lambda r: gen_full(r, 65, 2, 16), [F] * 5),
    "tail_257": (2, 16, lambda r: gen_full(r, 257, 2, 16), [F] * 5),
}
# the column-count splits: every column 2-3 bits, split 6+1, 6+2, 6+6+1
NARROW_SPLITS = {"cols_7": [6, 1], "cols_8": [6, 2], "cols_13": [6, 6, 1]}


def make_case(name):
    """(kw, vb, batch) of a consolidate case, deterministic per name."""
    kw, vb, gen, _ = CONSOLIDATE_CASES[name]
    seed = 1 + sorted(CONSOLIDATE_CASES).index(name)
    return kw, vb, gen(np.random.default_rng(seed))


def assert_case_shape(name, kw, vb, batch):
    """The planner shape the case exists for, asserted on its data."""
    shape = plan_shape(batch, kw, vb)
    want = CONSOLIDATE_CASES[name][3]
    if name in NARROW_SPLITS:
        assert [len(c) for c in shape] == NARROW_SPLITS[name], (name, shape)
        assert all(b in (2, 3) for c in shape for b in c), (name, shape)
    else:
        assert shape == want, (name, shape)
    assert len(batch[2]) <= 2000


# ------------------------------------------------- cached-plan sequences
#
# Device-staged inserts keep one cached sort plan per arrangement: the
# first batch primes it with padded bounds (pad_spans), later batches are
# sorted with the cached plan if it covers them and re-planned otherwise.
# Each sequence is a list of single-timestamp batches (kw = 1, vb = 8;
# batch i at time i) and the per-batch expectation "covered by the plan
# in force", asserted against the model by plan_trace.

def _seq_batch(rng, t, n, klo, khi, vlo, vhi):
    """Keys in [klo, khi], i64 vals in [vlo, vhi], ends planted."""
    keys = np.array([klo + int(x) for x in
                     rng.integers(0, khi - klo + 1, n, dtype=np.uint64)],
                    np.int64).reshape(n, 1)
    v = np.array([vlo + int(x) for x in
                  rng.integers(0, vhi - vlo + 1, n, dtype=np.uint64)],
                 np.int64)
    keys[0], keys[1], v[0], v[1] = klo, khi, vlo, vhi
    vals = v.view(np.uint8).reshape(n, 8).copy()
    batch = (keys, vals, np.full(n, t, np.uint64), _diffs(rng, n))
    return _mix(rng, batch)


def seq_high(rng):
    """Keys near INT64_MAX: the flipped values sit near 2^64 and the
    padded upper bound saturates to ~0; batch 1 reaches INT64_MAX itself,
    inside the padding and outside the exact bounds; batch 2 leaves."""
    return [(_seq_batch(rng, 0, 1200, I64_MAX - 1000, I64_MAX - 10, 0, 40),
             None),
            (_seq_batch(rng, 1, 1200, I64_MAX - 1100, I64_MAX, 0, 40), True),
            (_seq_batch(rng, 2, 1200, I64_MAX - 5000, I64_MAX, 0, 40),
             False)]


def seq_low(rng):
    """The mirror image: keys near INT64_MIN in the batch at time 0, the
    padded lower bound saturates to 0; vals (non-negative i64 near 0) do
    the same on a val word."""
    return [(_seq_batch(rng, 0, 1200, I64_MIN + 10, I64_MIN + 1000, 3, 900),
             None),
            (_seq_batch(rng, 1, 1200, I64_MIN, I64_MIN + 1100, 0, 1000),
             True),
            (_seq_batch(rng, 2, 1200, I64_MIN, I64_MIN + 5000, 0, 1000),
             False)]


def seq_const_then_wide(rng):
    """The val column is constant in the priming batch, constant at
    another value in the next (covered: no pass either way) and wide in
    the third (not covered: re-plan)."""
    return [(_seq_batch(rng, 0, 1200, -500, 500, 7, 7), None),
            (_seq_batch(rng, 1, 1200, -400, 400, -9, -9), True),
            (_seq_batch(rng, 2, 1200, -400, 400, I64_MIN, I64_MAX), False),
            (_seq_batch(rng, 3, 1200, -300, 300, I64_MIN, I64_MAX), True)]


def seq_pad_shift(rng):
    """A 31-bit val span beside a 33-bit key span: 64 bits exactly, one
    chunk; padded, the val span takes 32 bits and the layout splits."""
    k0, v0 = -2**31, 2**40
    return [(_seq_batch(rng, 0, 1200, k0, k0 + 2**32 + 9, v0,
                        v0 + 2**31 - 1), None),
            (_seq_batch(rng, 1, 1200, k0 - 1000, k0 + 2**32 + 1000, v0 - 99,
                        v0 + 2**31 + 99), True)]


PLAN_SEQUENCES = {"high": seq_high, "low": seq_low,
                  "const_then_wide": seq_const_then_wide,
                  "pad_shift": seq_pad_shift}


def make_sequence(name):
    seed = 100 + sorted(PLAN_SEQUENCES).index(name)
    return PLAN_SEQUENCES[name](np.random.default_rng(seed))


def plan_trace(seq):
    """Walk a sequence through the cache model: asserts each batch's
    covered / not-covered expectation, returns per batch (exact shape,
    shape of the plan it is sorted with)."""
    cached, out = None, []
    for batch, want_covered in seq:
        spans = column_spans(batch, 1, 8)
        if cached is None:
            assert want_covered is None
            cached = pad_spans(spans)
        else:
            assert covered(cached, spans) == want_covered
            if not want_covered:
                cached = pad_spans(spans)
        out.append((chunk_bits(spans), chunk_bits(cached)))
    return out


# ------------------------------------- reduce: SUM_I64 + COUNT, big ints

def sum_count_spec(abi, kw):
    """SUM_I64 then COUNT over the i64 at val offset 0 (vb = 8)."""
    aggs = [abi.Aggregate(func=f, off=0, width=8, is_float=0, nullable=0)
            for f in (abi.MZ_AGG_SUM_I64, abi.MZ_AGG_COUNT)]
    return abi.reduce_spec(aggs, abi.schema(kw, 8))


class SumCountModel:
    """The accumulable reduce over Python integers: per key the sum of
    val * diff mod 2^128, the count and the total mod 2^64. push() returns
    the corrections (new minus old finalized rows per changed key and
    time, in time order) as consolidated rows of to_rows' form, the
    48-byte output val being two 24-byte slots {null byte, pad, 16-byte
    value}."""

    def __init__(self):
        self.state = {}

    @staticmethod
    def _row(st):
        acc, nn, total = st
        if wrap_i64(total) > 0 and acc == 0 and nn == 0:
            s = bytes([1]) + bytes(23)
        else:
            s = bytes(8) + acc.to_bytes(16, "little")
        return s + bytes(8) + nn.to_bytes(8, "little") + bytes(8)

    def push(self, batch, kw):
        out = []
        rows = to_rows(*batch, kw, 8)
        for t in sorted({r[2] for r in rows}):
            olds = {}
            for k, v, rt, d in rows:
                if rt != t:
                    continue
                acc, nn, total = self.state.get(k, (0, 0, 0))
                olds.setdefault(k, (acc, nn, total))
                x = wrap_i64(v[0])
                self.state[k] = ((acc + x * d) % 2**128, (nn + d) % M64,
                                 (total + d) % M64)
            for k, old in olds.items():
                new = self.state[k]
                oe, ne = any(old), any(new)
                if oe and ne and self._row(old) == self._row(new):
                    continue
                if oe:
                    out.append((k, canon_val_key(self._row(old)), t, -1))
                if ne:
                    out.append((k, canon_val_key(self._row(new)), t, 1))
                else:
                    del self.state[k]
        return naive.consolidate(out)


def gen_time_major(rng, n=1500):
    """One multi-timestamp reduce input: kw = 2 keys from a pool of 120
    full-width pairs (extremes planted), times spread over {0, 2^40, 2^63,
    2^64 - 2}, i64 vals with the extremes among them."""
    pool = _u64(rng, 240).view(np.int64).reshape(120, 2)
    pool[0], pool[1] = (I64_MIN, I64_MAX), (I64_MAX, I64_MIN)
    pool[2], pool[3] = (I64_MIN, I64_MIN), (I64_MAX, I64_MAX)
    pool[4], pool[5] = (-1, 0), (0, -1)
    keys = pool[rng.integers(0, 120, n)]
    keys[:4] = pool[:4]
    times = rng.choice(np.array([0, 2**40, 2**63, 2**64 - 2], np.uint64), n)
    times[:4] = [0, 2**40, 2**63, 2**64 - 2]
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    v[::7] = rng.choice(np.array([I64_MIN, I64_MAX], np.int64), len(v[::7]))
    vals = v.view(np.uint8).reshape(n, 8).copy()
    return keys, vals, times, _diffs(rng, n)


def gen_sum_extremes(rng, t, n=200):
    """One single-timestamp push: 8 keys (extremes among them), vals
    INT64_MIN / INT64_MAX, diffs +-1 and +-2^62."""
    pool = np.array([I64_MIN, I64_MAX, -1, 0, 1, 2**40, -2**40, 77],
                    np.int64)
    keys = rng.choice(pool, (n, 1))
    v = rng.choice(np.array([I64_MIN, I64_MAX], np.int64), n)
    diffs = rng.choice(np.array([1, -1, 2**62, -2**62], np.int64), n)
    return (keys, v.view(np.uint8).reshape(n, 8).copy(),
            np.full(n, t, np.uint64), diffs)


# --------------------------------------------- probes over full-width keys

def gen_probe_arrangement(rng, kw):
    """Two batches (vb = 8) for one arrangement: full-width keys and the
    sign-boundary keys. Times stay below 2^64 - 2 so the batch bounds
    [0, 2^64 - 1) are honest."""
    a = gen_full(rng, 1200, kw, 8)
    b = gen_sign(rng, 800, kw)
    np.minimum(a[2], np.uint64(U64_MAX - 2), out=a[2])
    return [a, b]


def gen_probe_stream(rng, batches, kw):
    """Stream rows (vb = 0) at times 3, 2^63 and 2^64 - 3, the first and
    the last of which occur in the arrangement (so t' <= t and t' < t
    differ): 150 keys present in the arrangement, the extremes, and 50
    absent keys. The all-INT64_MAX key probes at the arrangement's own
    last time."""
    present = np.concatenate([b[0] for b in batches])
    keys = np.unique(np.concatenate([
        present[rng.choice(len(present), 150, replace=False)],
        np.full((1, kw), I64_MIN), np.full((1, kw), I64_MAX),
        _u64(rng, 50 * kw).view(np.int64).reshape(50, kw)]), axis=0)
    n = len(keys)
    times = rng.choice(np.array([3, 2**63, U64_MAX - 2], np.uint64), n)
    times[-1] = U64_MAX - 2  # unique() sorted the all-INT64_MAX key last
    p = rng.permutation(n)
    return (keys[p], np.zeros((n, 0), np.uint8), times[p],
            rng.choice(np.array([-2, 1, 3], np.int64), n))


def naive_halfjoin(stream, batches, kw, le):
    """Half join through naive.join_full: per stream time t, the stream
    rows at t against the arrangement rows at t' <= t (le) or t' < t;
    the output row is (key, lookup val, t, product of the diffs)."""
    arr = [r for b in batches for r in to_rows(*b, kw, 8)]
    srows = to_rows(*stream, kw, 0)
    out = []
    for t in sorted({r[2] for r in srows}):
        seen = [r for r in arr if (r[2] <= t if le else r[2] < t)]
        joined = naive.join_full([r for r in srows if r[2] == t], seen)
        assert all(jt == t for _, _, jt, _ in joined)
        out += [(k, v2, jt, d) for k, (_, v2), jt, d in joined]
    return naive.consolidate(out)


def probe_closure(abi, kw):
    """Identity probe: out key = the key, out val = the lookup's val."""
    return abi.closure([], [abi.field(abi.MZ_SRC_KEY, 0, 8 * kw)],
                       [abi.field(abi.MZ_SRC_VAL_LOOKUP, 0, 8)],
                       abi.schema(kw, 8))


# ------------------------------------------------ keys that wrap a table

def wrap_keys(kw=1, first_word=0, nbits=12, tail=3, scan_bits=22):
    """Keys (int64 [m, kw]) whose route hash has its low `nbits` bits in
    the last `tail` values: in any table of <= 2^nbits slots they all
    land in the last `tail` slots, so a cluster of more than `tail` of
    them runs off the end and wraps to slot 0. Scans 2^scan_bits
    consecutive values of the last key word."""
    from materialize_amd.dist import route_hash
    scan = np.arange(-2**(scan_bits - 1), 2**(scan_bits - 1), dtype=np.int64)
    keys = np.empty((len(scan), kw), np.int64)
    keys[:, :kw - 1] = first_word
    keys[:, kw - 1] = scan
    low = route_hash(keys, kw) & np.uint64(2**nbits - 1)
    return keys[low >= np.uint64(2**nbits - tail)]
