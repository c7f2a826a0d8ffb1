"""Cost of a temporal-filter push ("Temporal filter").

A sliding window `mz_now() >= ts AND mz_now() < ts + W` over a stream of
(key, [ts, x]) rows: step s pushes --rows fresh device-resident rows at time
s with bounds [s, s + 1), their ts drawn from {s - 1, s, s + 1} ("near the
current time"), keys and x random, so no two rows consolidate. Every row
puts its -1 at ts + W into the held buffer (and, for ts = s + 1, its +1
too), and every push releases what W steps ago left there: in steady state
the buffer holds about W * rows updates, all of which the push consolidates
again.

Per (rows, W) point: W + 2 warm-up pushes reach the steady state, then the
median host-clock time of --calls pushes (each ends in the engine's own
closing readback; out-batches are released without copying them to the
host), then, from --calls more pushes with kernel timing on, the device-event
time of k_temporal_eval alone, and the held row count and the last push's
out rows. Prints one JSON line. Needs a GPU: there is no fallback.

    python profiles/temporal_cost.py [--rows 100000 1000000] [--windows 2 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="+",
                   default=[100_000, 1_000_000])
    p.add_argument("--windows", type=int, nargs="+", default=[2, 64])
    p.add_argument("--calls", type=int, default=8)
    p.add_argument("--seed", type=int, default=11)
    args = p.parse_args()

    import torch
    from materialize_amd import _abi as abi
    from materialize_amd import render
    from materialize_amd._ffi import GpuCtx

    if not torch.cuda.is_available():
        raise SystemExit("temporal_cost: no GPU")
    dev = torch.device("cuda:0")
    g = GpuCtx()
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    sch = abi.schema(1, 16)
    VS = abi.MZ_SRC_VAL_STREAM

    def point(n, w):
        bounds = [abi.time_bound(abi.MZ_CMP_GE, VS, 0),
                  abi.time_bound(abi.MZ_CMP_LT, VS, 0, add=w)]
        op = render.render_temporal_filter(
            g, render.TemporalFilterPlan(abi.temporal_spec(sch, bounds)))
        diffs = torch.ones(n, dtype=torch.int64, device=dev)
        step = [2]

        def push():
            s = step[0]
            step[0] += 1
            keys = torch.randint(0, 2**40, (n,), dtype=torch.int64,
                                 device=dev, generator=gen)
            vals = torch.randint(0, 2**40, (n, 2), dtype=torch.int64,
                                 device=dev, generator=gen)
            vals[:, 0] = s + torch.randint(-1, 2, (n,), dtype=torch.int64,
                                           device=dev, generator=gen)
            times = torch.full((n,), s, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            u = abi.make_updates_from_torch(
                keys, vals.view(torch.uint8).reshape(-1), times, diffs, s,
                s + 1)
            t0 = time.perf_counter()
            out = op.push(u)
            ms = (time.perf_counter() - t0) * 1e3
            rows = out.n
            out.release()
            return ms, rows

        for _ in range(w + 2):
            push()
        ms = [push()[0] for _ in range(args.calls)]
        g.set_kernel_timing(True)
        g.probe_stats()
        kms = []
        for _ in range(args.calls):
            _, rows = push()
            kms.append(g.probe_stats()[0])
        g.set_kernel_timing(False)
        held, next_time, frontier = op.stats()
        op.drop()
        return {"rows_per_push": n, "window_steps": w,
                "pushes": step[0] - 2, "held_rows": held,
                "out_rows_last_push": rows,
                "push_median_ms": round(statistics.median(ms), 3),
                "push_min_ms": round(min(ms), 3),
                "push_max_ms": round(max(ms), 3),
                "eval_kernel_median_ms": round(statistics.median(kms), 4),
                "eval_kernel_min_ms": round(min(kms), 4),
                "eval_kernel_max_ms": round(max(kms), 4)}

    res = {"calls": args.calls,
           "points": [point(n, w) for n in args.rows for w in args.windows]}
    print(json.dumps(res))
    g.close()


if __name__ == "__main__":
    main()
