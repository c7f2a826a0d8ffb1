"""Cost of a peek with a key range and a finishing ("Peek
select").

One arrangement of 1-word keys and 16-byte vals [a i64][b i64] is built from
--batches device-resident inserts of --rows random rows each (times 0, 1,
...), as profiles/peek_scan_cost.py builds it. `SELECT * FROM idx WHERE k >=
0 AND k < hi ORDER BY a DESC LIMIT n` is then answered two ways, as of the
last time, for every range in --fractions (of the key space) and every limit
in --limits (0 = none):

  host    what a caller does without the entry point: mz_gpu_peek_scan of
          the whole arrangement, the out-batch copied to the host, then the
          range filter, a stable numpy sort and the slice there
  select  mz_gpu_peek_select with the range and the finishing, its
          out-batch copied to the host

and, per range, `walk`: mz_gpu_peek_select with the range alone, its
out-batch released on the device — what the scan and its consolidation cost
before any finishing, so that select minus walk at a small limit is the
finishing's share.

mz_gpu_peek_scan does not change with mz_gpu_peek_select, so both ways run
in one process, interleaved per shape. Per way and shape: the median
host-clock time of --calls calls after --warmup; every call ends with the
result in host memory. The two results are compared once per shape. Prints
one JSON line. Needs a GPU: there is no fallback.

    python profiles/peek_select_cost.py [--rows 1000000] [--batches 6]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def host_finish(cols, hi, limit):
    """WHERE k < hi ORDER BY a DESC LIMIT limit (0 = none) over the host
    columns of a whole-arrangement peek, in numpy."""
    import numpy as np
    k, v, t, d = cols
    keep = np.nonzero(k < hi)[0]  # keys are >= 0
    a = v.reshape(-1, 16)[keep, :8].copy().view(np.int64).ravel()
    # rows arrive in canonical order: a stable sort keeps the tie-break
    keep = keep[np.argsort(-a, kind="stable")]
    d = d[keep]
    if limit:
        hi_pos = np.cumsum(d)
        lo_pos = hi_pos - d
        m = int(np.searchsorted(lo_pos, limit, side="left"))
        keep, d = keep[:m], np.minimum(hi_pos[:m], limit) - lo_pos[:m]
    return k[keep], v.reshape(-1, 16)[keep].ravel(), t[keep], d


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--batches", type=int, default=6)
    p.add_argument("--keys", type=int, default=2_000_000)
    p.add_argument("--fractions", type=float, nargs="+",
                   default=[0.0001, 0.01, 1.0])
    p.add_argument("--limits", type=int, nargs="+", default=[10, 1000, 0])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--seed", type=int, default=11)
    args = p.parse_args()

    import numpy as np
    import torch
    from materialize_amd import _abi as abi
    from materialize_amd._ffi import GpuCtx

    if not torch.cuda.is_available():
        raise SystemExit("peek_select_cost: no GPU")
    dev = torch.device("cuda:0")
    g = GpuCtx()
    arr = g.arr_create(abi.schema(1, 16))
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    n = args.rows
    diffs = torch.ones(n, dtype=torch.int64, device=dev)
    for t in range(args.batches):
        keys = torch.randint(0, args.keys, (n,), dtype=torch.int64,
                             device=dev, generator=gen)
        vals = torch.randint(-2**62, 2**62, (n, 2), dtype=torch.int64,
                             device=dev, generator=gen)
        times = torch.full((n,), t, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        g.arr_insert(arr, abi.make_updates_from_torch(
            keys, vals.view(torch.uint8).reshape(-1), times, diffs, t, t + 1))
    n_batches, n_updates, hbm_bytes = g.arr_stats(arr)
    as_of = args.batches - 1
    order = [abi.order_by(abi.MZ_SRC_VAL_LOOKUP, 0, desc=True)]

    def host(hi, limit):
        out = g.peek_scan_dev(arr, as_of)
        cols = out.to_host()
        out.release()
        return host_finish(cols, hi, limit)

    def select(hi, limit):
        rng = abi.key_range(lo=0, hi=hi, hi_inclusive=False)
        fin = abi.finishing(order, limit=limit or None)
        return g.peek_select(arr, as_of, rng, None, fin)

    def walk(hi, limit):
        rng = abi.key_range(lo=0, hi=hi, hi_inclusive=False)
        out = g.peek_select_dev(arr, as_of, rng)
        rows = out.n
        out.release()
        return rows

    def measure(call, hi, limit):
        for _ in range(args.warmup):
            res = call(hi, limit)
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call(hi, limit)
            ms.append((time.perf_counter() - t0) * 1e3)
        return res, {"median_ms": round(statistics.median(ms), 3),
                     "min_ms": round(min(ms), 3),
                     "max_ms": round(max(ms), 3)}

    res = {"rows_per_batch": n, "inserts": args.batches,
           "spine_batches": n_batches, "updates": n_updates,
           "arr_hbm_bytes": hbm_bytes, "as_of": as_of,
           "warmup": args.warmup, "calls": args.calls, "shapes": []}
    for frac in args.fractions:
        hi = max(1, int(args.keys * frac))
        _, tw = measure(walk, hi, 0)
        for limit in args.limits:
            want, th = measure(host, hi, limit)
            got, ts = measure(select, hi, limit)
            scanned, matched = g.last_peek_stats
            for a, b in zip(got, want):
                assert np.array_equal(np.asarray(a).view(np.uint8),
                                      np.asarray(b).view(np.uint8)), \
                    (frac, limit)
            res["shapes"].append({
                "key_fraction": frac, "limit": limit or None,
                "scanned_vals": scanned, "rows_matched": matched,
                "out_rows": len(got[3]), "host": th, "select": ts,
                "walk": tw,
                "ratio_host_over_select":
                    round(th["median_ms"] / ts["median_ms"], 2)})
    print(json.dumps(res))
    g.close()


if __name__ == "__main__":
    main()
