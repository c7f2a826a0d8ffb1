"""Cost of a window-function push beside a TopK push ("Window
functions").

Device-resident input. Per --rows point R: both operators are loaded with
4 R rows (key = i mod R/16, so partitions of about 64 rows; val = one i64 x,
unique; diff 1) at time 0. Then every churn push, at a time of its own,
retracts R/2 of the loaded rows and inserts R/2 new ones under random keys,
so it changes nearly every partition and never drives a count negative.

The same churn goes through mz_gpu_window_push with [ROW_NUMBER, LAG(x, 1)]
ordered by x, and through mz_gpu_topk_push ordered by x with no limit. TopK
does the same probe, install, probe and sort work and differs only in what
it emits (the kept rows, where the window operator writes one row per
position of every changed partition, 25 bytes wide), so it is the
yardstick. The two alternate in one process: 2 warm-up pushes each, then
--calls timed ones, host clock around the call (both end in the engine's own
synchronisation; out-batches are released without copying them to the host).

--aggregates puts a window-aggregate spec in the window operator's place,
same churn and same yardstick: [SUM(x) over the default frame (the running
total), SUM(x) and COUNT(*) over ROWS 2 PRECEDING..CURRENT ROW, MAX(x) over
the partition], 43 bytes wide. It adds the prefix scans (one 128-bit, one
by partition) to each of the two evaluations of a push and two searches per
ROWS function to every output row.
Prints one JSON line. Needs a GPU: there is no fallback.

    python profiles/window_cost.py [--rows 100000 400000] [--calls 5]
                                   [--aggregates]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP = 2


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="+", default=[100_000, 400_000])
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--seed", type=int, default=11)
    p.add_argument("--aggregates", action="store_true")
    args = p.parse_args()
    if args.calls + WARMUP > 8:
        raise SystemExit("window_cost: --calls at most 6 (the loaded rows "
                         "last for 8 pushes)")

    import ctypes as C

    import torch
    from materialize_amd import _abi as abi
    from materialize_amd._ffi import GpuCtx

    if not torch.cuda.is_available():
        raise SystemExit("window_cost: no GPU")
    dev = torch.device("cuda:0")
    g = GpuCtx()
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    sch = abi.schema(1, 8)
    order = [(0, 8, False)]
    if args.aggregates:
        moving = dict(start=abi.preceding(2), end=abi.CURRENT_ROW)
        funcs = [abi.wf_sum(0, 8), abi.wf_sum(0, 8, **moving),
                 abi.wf_count(**moving),
                 abi.wf_max(0, 8, frame=abi.MZ_WF_FRAME_PARTITION)]
    else:
        funcs = [abi.wf_row_number(), abi.wf_lag(0, 8, 1)]
    wspec = abi.window_spec(sch, order, funcs)
    tspec = abi.topk_spec(sch, order, offset=0, limit=-1)

    def stats(ms, what):
        return {f"{what}_median_ms": round(statistics.median(ms), 3),
                f"{what}_min_ms": round(min(ms), 3),
                f"{what}_max_ms": round(max(ms), 3)}

    def point(n):
        parts, half, base = max(n // 16, 1), n // 2, 4 * n
        win = g.window_create(wspec)
        topk = g.topk_create(tspec)

        def updates(keys, x, diffs, t):
            times = torch.full_like(x, t)
            torch.cuda.synchronize()
            return abi.make_updates_from_torch(
                keys, x.view(torch.uint8).reshape(-1), times, diffs, t, t + 1)

        def push_window(u):
            t0 = time.perf_counter()
            out = g.window_push_dev(win, u)
            ms = (time.perf_counter() - t0) * 1e3
            rows = out.n
            out.release()
            return ms, rows

        def push_topk(u):
            outp = C.POINTER(abi.OutBatch)()
            t0 = time.perf_counter()
            g._check(g.lib.mz_gpu_topk_push(g.ctx, topk, C.byref(u),
                                            C.byref(outp)))
            ms = (time.perf_counter() - t0) * 1e3
            rows = int(outp.contents.n)
            g.lib.mz_gpu_out_release(g.ctx, outp)
            return ms, rows

        x0 = torch.arange(base, dtype=torch.int64, device=dev)
        load = updates(x0 % parts, x0, torch.ones_like(x0), 0)
        load_w, _ = push_window(load)
        load_t, _ = push_topk(load)
        ms_w, ms_t, rows_w, rows_t = [], [], 0, 0
        for s in range(WARMUP + args.calls):
            gone = x0[s * half:(s + 1) * half]
            new = base + s * half + torch.arange(half, dtype=torch.int64,
                                                 device=dev)
            keys = torch.cat([gone % parts, torch.randint(
                0, parts, (half,), dtype=torch.int64, device=dev,
                generator=gen)])
            diffs = torch.cat([-torch.ones_like(gone), torch.ones_like(new)])
            u = updates(keys, torch.cat([gone, new]), diffs, s + 1)
            w, rows_w = push_window(u)
            k, rows_t = push_topk(u)
            if s >= WARMUP:
                ms_w.append(w)
                ms_t.append(k)
        g.window_drop(win)
        g.lib.mz_gpu_topk_drop(g.ctx, topk)
        return dict(rows=n, loaded_rows=base, partitions=parts,
                    load_window_ms=round(load_w, 3),
                    load_topk_ms=round(load_t, 3),
                    window_out_rows=rows_w, topk_out_rows=rows_t,
                    **stats(ms_w, "window_push"), **stats(ms_t, "topk_push"))

    res = {"calls": args.calls,
           "window_spec": "aggregates" if args.aggregates else "rank_lag",
           "points": [point(n) for n in args.rows]}
    print(json.dumps(res))
    g.close()


if __name__ == "__main__":
    main()
