"""Per-push cost of a DISTINCT aggregate ("Cost of DISTINCT").

Two reduce operators on one context are fed the same device-resident
pushes: `COUNT(DISTINCT a), SUM(a)` and the same spec with the flag
cleared. Each push is --rows fresh rows at a new single timestamp over
--keys keys, `a` drawn from --datums values (so the pair tables stay below
their initial capacity and never rebuild inside the window). The pushes
alternate between the operators; the time is the host clock around one push,
which ends in the operator's own closing device synchronize. Prints one JSON
line. Needs a GPU: there is no fallback.

    python profiles/distinct_cost.py [--rows 1000000] [--keys 100000]
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
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--keys", type=int, default=100_000)
    p.add_argument("--datums", type=int, default=16)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--pushes", type=int, default=20)
    p.add_argument("--seed", type=int, default=7)
    args = p.parse_args()

    import torch
    from materialize_amd import _abi as abi
    from materialize_amd._ffi import GpuCtx

    if not torch.cuda.is_available():
        raise SystemExit("distinct_cost: no GPU")
    dev = torch.device("cuda:0")
    g = GpuCtx()
    sch = abi.schema(1, 8)

    def spec(distinct):
        return abi.reduce_spec(
            [abi.Aggregate(func=abi.MZ_AGG_COUNT, off=0, width=8, is_float=0,
                           nullable=0, distinct=distinct),
             abi.Aggregate(func=abi.MZ_AGG_SUM_I64, off=0, width=8,
                           is_float=0, nullable=0)], sch)

    ops = {"distinct": g.reduce_create(spec(1)),
           "plain": g.reduce_create(spec(0))}
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    n = args.rows
    diffs = torch.ones(n, dtype=torch.int64, device=dev)
    ms = {name: [] for name in ops}
    out_rows = {}
    for step in range(args.warmup + args.pushes):
        keys = torch.randint(0, args.keys, (n,), dtype=torch.int64,
                             device=dev, generator=gen)
        a = torch.randint(0, args.datums, (n,), dtype=torch.int64,
                          device=dev, generator=gen)
        times = torch.full((n,), step, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for name, op in ops.items():
            u = abi.make_updates_from_torch(keys, a.view(torch.uint8), times,
                                            diffs, step, step + 1)
            t0 = time.perf_counter()
            out = g.reduce_push_dev(op, u)
            dt = (time.perf_counter() - t0) * 1e3
            out_rows[name] = out.n
            out.release()
            if step >= args.warmup:
                ms[name].append(dt)

    def summary(v):
        return {"median_ms": round(statistics.median(v), 3),
                "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    res = {"rows": n, "keys": args.keys, "datums": args.datums,
           "warmup": args.warmup, "pushes": args.pushes,
           "distinct": summary(ms["distinct"]), "plain": summary(ms["plain"]),
           "last_out_rows": out_rows}
    res["ratio_median"] = round(res["distinct"]["median_ms"] /
                                res["plain"]["median_ms"], 3)
    print(json.dumps(res))
    for op in ops.values():
        g.reduce_drop(op)
    g.close()


if __name__ == "__main__":
    main()
