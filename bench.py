#!/usr/bin/env python3
"""bench.py — TPC-H Q3 incremental maintenance on MI355X.

Metric (BASELINE.json): input update rows/sec maintained (TPC-H Q3 delta
join). A step = one churn batch (retract/insert order + lineitem rows,
tpch.rs:204-241 shape) maintained end-to-end: arrangement pushes, the
orders + lineitem delta paths (2 probe stages each) and the SUM reduce.

N=1 workload = BASELINE config 2: TPC-H SF1 Q3 under 100k-row churn
batches on one GPU. N>1 = config 3 (weak scaling): SF 1.25*N sharded by
key hash across N GPUs with all-to-all-v exchanges over RCCL/xGMI,
batches of 100k*N global rows.

Inputs are pre-generated and pre-staged into HBM before the timed region
(churn columns as torch CUDA tensors); the PCIe-inclusive rate is noted
in DESIGN.md §7, never reported as `value`.

Contract: W untimed warmup steps, then exactly K timed steps bracketed by
barrier + torch.cuda.synchronize on both sides; MAX over ranks; rank 0
prints ONE JSON line.

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print the line. `--full` adds the legs that take runs
of their own (today: the CPU-oracle baseline, reported as `cpu_baseline`,
null in a plain run). `--dump-outputs DIR` writes what the last timed
step returned to its caller (see dump_outputs) for build-to-build
comparison; inputs depend only on the arguments (seeded generator).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12  # B/s, MI355X spec (MI355X_MICROARCH.md)
METRIC = "input update rows/sec maintained (TPC-H Q3 delta join)"


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    # defaults span the full merge hierarchy (pool merges every ~6 steps,
    # the giant run-fold every ~30): shorter windows undersample the
    # amortized merges and overstate rows/s
    p.add_argument("--steps", type=int, default=36)
    p.add_argument("--warmup", type=int, default=6)
    p.add_argument("--sf", type=float, default=0.0, help="0 = auto by N")
    p.add_argument("--batch-rows", type=int, default=0, help="0 = auto")
    p.add_argument("--full", action="store_true",
                   help="also run the legs beyond the headline figure "
                        "(the CPU-oracle baseline); off by default")
    p.add_argument("--no-cpu-baseline", action="store_true",
                   help="with --full: skip the CPU-oracle baseline leg")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last timed "
                        "step's outputs as DIR/<name>.npy (float64)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--call-profile", action="store_true",
                   help="print per-engine-call wall time breakdown")
    p.add_argument("--no-pipeline", action="store_true",
                   help="disable the 1-deep insert pipeline (A/B control)")
    p.add_argument("--workload", default="q3", choices=["q3", "q17"],
                   help="q3 = BASELINE config 2/3 (default, the metric's "
                        "workload); q17 = config 5 shape at N=1")
    p.add_argument("--backend", default="nccl",
                   help="torch.distributed backend for N>1 (nccl = RCCL; "
                        "gloo only for single-box validation)")
    return p.parse_args()


class CallProfiler:
    """Wraps an engine ctx's methods with wall-time accumulation."""

    METHODS = ["consolidate_dev", "arr_push", "arr_insert",
               "halfjoin_dev", "reduce_push_dev", "reduce_push2_dev",
               "join_push", "arr_maintain"]

    def __init__(self, ctx):
        self.t = {m: [0.0, 0] for m in self.METHODS}
        for m in self.METHODS:
            orig = getattr(ctx, m)

            def wrap(orig=orig, m=m):
                def f(*a, **kw):
                    t0 = time.perf_counter()
                    r = orig(*a, **kw)
                    self.t[m][0] += time.perf_counter() - t0
                    self.t[m][1] += 1
                    return r
                return f
            setattr(ctx, m, wrap())

    def report(self, steps):
        for m, (tt, calls) in sorted(self.t.items(), key=lambda x: -x[1][0]):
            print(f"#   {m:18s} {tt*1e3:9.2f} ms total  {calls:5d} calls  "
                  f"{tt*1e3/max(steps,1):7.2f} ms/step", file=sys.stderr)


DUMP_MAX_BYTES = 64 << 20


def _words_f64(a, n):
    """Raw little-endian column bytes -> [n, words] float64 of their
    uint32 words (exact: every word < 2^32)."""
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if n == 0:
        return np.zeros((0, 0), np.float64)
    return a.view("<u4").reshape(n, -1).astype(np.float64)


def dump_outputs(dirname, cols, rank=0, world=1):
    """Write one out-batch (keys, vals, times, diffs as the engine's
    to_host() returns them; None = the step produced no output) as
    float64 .npy files: `keys`/`vals` are the rows' raw bytes as uint32
    words (lossless for any 64-bit content), `times`/`diffs` the values
    themselves, `n_rows` the full row count. Above 64 MB in all a fixed
    seeded row sample (ascending row order) is written and `sample_rows`
    holds the chosen row indices."""
    os.makedirs(dirname, exist_ok=True)
    if cols is None:
        cols = (np.empty(0, np.uint64), np.empty(0, np.uint8),
                np.empty(0, np.uint64), np.empty(0, np.int64))
    keys, vals, times, diffs = cols
    n = len(times)
    arrs = {"keys": _words_f64(keys, n), "vals": _words_f64(vals, n),
            "times": np.asarray(times).astype(np.float64),
            "diffs": np.asarray(diffs).astype(np.float64)}
    # float64 per row: key + val words, time, diff, sample_rows entry;
    # 4 KB of headroom for the .npy headers and n_rows
    row_bytes = 8 * (arrs["keys"].shape[1] + arrs["vals"].shape[1] + 3)
    cap = (DUMP_MAX_BYTES - 4096) // row_bytes
    if n > cap:
        pick = np.sort(np.random.default_rng(0).choice(n, cap,
                                                       replace=False))
        arrs = {k: a[pick] for k, a in arrs.items()}
        arrs["sample_rows"] = pick.astype(np.float64)
    arrs["n_rows"] = np.array([n], np.float64)
    sfx = "" if world == 1 else f"_rank{rank}"
    for name, a in arrs.items():
        np.save(os.path.join(dirname, f"{name}{sfx}.npy"), a)


def stage_churn(churn, t, device):
    """Pre-stage one churn batch's columns into HBM as torch tensors and
    build device Updates descriptors (times == t)."""
    import torch
    from materialize_amd import _abi as abi
    out = {}
    name_map = {"orders_by_cust": "orders_by_custkey",
                "orders": "orders_by_orderkey",
                "lineitem": "lineitem"}
    for name, (keys, vals, diffs) in churn.items():
        if name not in name_map:  # relations outside this workload
            continue
        tgt = name_map[name]
        n = len(keys)
        kt = torch.from_numpy(np.ascontiguousarray(keys, np.int64)
                              ).to(device)
        vt = torch.from_numpy(np.ascontiguousarray(vals, np.uint8).reshape(-1)
                              ).to(device)
        tt = torch.full((n,), t, dtype=torch.int64, device=device)
        dt = torch.from_numpy(np.ascontiguousarray(diffs, np.int64)
                              ).to(device)
        out[tgt] = abi.make_updates_from_torch(kt, vt, tt, dt, t, t + 1)
    return out


def filter_shard(churn, world, rank):
    """Pre-filter churn columns to this rank's shard (untimed; the
    generator is deterministic and identical on every rank)."""
    from materialize_amd.dist import shard_of
    if world == 1:
        return churn
    out = {}
    for name, (keys, vals, diffs) in churn.items():
        keys = np.ascontiguousarray(keys, np.int64)
        vals = np.ascontiguousarray(vals, np.uint8).reshape(len(keys), -1)
        m = shard_of(keys, 1, world) == rank
        out[name] = (keys[m], vals[m], diffs[m])
    return out


def run_cpu_baseline(seed, cores=0, batch=100_000, steps=0, sf=1.0):
    """Oracle (the CPU restatement, kind 'port') on a bounded sample of the
    SAME workload shape as the GPU run: TPC-H Q3 churn batches on the
    box's host cores — sharded oracle dataflows on worker threads with an
    in-process exchange (the thread analog of timely workers; the oracle's
    C calls release the GIL). Runs 1/4/8 worker threads, each over a
    >=2 s timed window (step counts sized from a probe run), and reports
    the best as `value` with every worker count's figure in
    `per_workers`."""
    import copy
    import math
    import threading
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from materialize_amd.tpch import TpchGen
    from materialize_amd.thread_exchange import ThreadExchangeGroup
    from materialize_amd.workloads import ShardedQ3Dataflow
    from pyoracle import OracleCtx

    MIN_WINDOW = float(os.environ.get("MZ_CPU_BASELINE_WINDOW", "2.0"))
    gen = TpchGen(sf=sf, seed=seed)
    base = copy.deepcopy(gen.__dict__)  # t=0 snapshot for load()
    churns = []

    def ensure(n):
        while len(churns) < n:
            churns.append(gen.churn(batch))

    def run(W, nsteps):
        ensure(nsteps + 1)
        gen.__dict__.update(base)  # load() reads the t=0 state
        group = ThreadExchangeGroup(W)
        results = [None] * W

        def worker(rank):
            df = ShardedQ3Dataflow(OracleCtx(), group.member(rank))
            df.load(gen)
            r, corr = df.step(churns[0], 1)  # warmup
            if corr is not None:
                corr.release()
            group.barrier.wait()
            t0 = time.perf_counter()
            total = 0
            for i in range(1, nsteps + 1):
                r, corr = df.step(churns[i], i + 1)
                if corr is not None:
                    corr.release()
                total += r
            group.barrier.wait()
            results[rank] = (total, time.perf_counter() - t0)

        threads = [threading.Thread(target=worker, args=(r,))
                   for r in range(W)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        total = results[0][0]
        dt = max(r[1] for r in results)
        return total / dt, dt

    ncpu = os.cpu_count() or 1
    worker_counts = [w for w in (1, 4, 8) if w <= max(ncpu, 1)] or [1]
    if cores:
        worker_counts = sorted(set(worker_counts + [cores]))
    # probe (1 worker, 2 steps) sizes each window to >= MIN_WINDOW
    v_probe, _ = run(1, 2)
    per = {}
    best = (0.0, 1, 0.0, 0)
    last_v, last_w = v_probe, 1
    for W in worker_counts:
        # size from the last measured rate (scaling is sublinear; a
        # linear estimate inflated the 8-worker window 10x)
        est = max(last_v * min(W / last_w, 1.6), 1.0)
        nsteps = min(max(int(math.ceil(MIN_WINDOW * est / batch)) + 1, 3),
                     240)
        v, dt = run(W, nsteps)
        if dt < MIN_WINDOW:  # estimate undershot: redo with scaled steps
            nsteps = min(int(math.ceil(nsteps * (MIN_WINDOW / dt) * 1.2)),
                         240)
            v, dt = run(W, nsteps)
        per[str(W)] = {"rows_s": v, "window_s": round(dt, 2),
                       "steps": nsteps}
        last_v, last_w = v, W
        if v > best[0]:
            best = (v, W, dt, nsteps)
    return {
        "value": best[0],
        "unit": "rows/s",
        "cores": best[1],
        "kind": "port",
        "per_workers": per,
        "sample": (f"oracle C++ restatement, TPC-H SF{sf:g} Q3 churn "
                   f"batches of ~{batch} rows; sharded worker threads "
                   f"with in-process exchange; per-worker-count windows "
                   f">= {MIN_WINDOW:g}s (see per_workers); best = "
                   f"{best[1]} workers over {best[2]:.1f}s"),
    }


def run_cpu_baseline_q17(seed, batch, steps=3, sf=1.0):
    """Oracle Q17 dataflow on one host core, bounded sample."""
    import copy
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from materialize_amd.tpch import TpchGen
    from materialize_amd.workloads import Q17Dataflow
    from pyoracle import OracleCtx
    gen = TpchGen(sf=sf, seed=seed)
    base = copy.deepcopy(gen.__dict__)
    churns = [gen.churn(batch) for _ in range(steps + 1)]
    gen.__dict__.update(base)
    df = Q17Dataflow(OracleCtx())
    df.load(gen)
    df.step(churns[0], 1)  # warmup
    t0 = time.perf_counter()
    total = 0
    for i in range(1, steps + 1):
        total += df.step(churns[i], i + 1)
    dt = time.perf_counter() - t0
    return {
        "value": total / dt, "unit": "rows/s", "cores": 1, "kind": "port",
        "sample": (f"oracle C++ restatement, TPC-H SF{sf:g} Q17, {steps} "
                   f"churn batches of ~{batch} rows, 1 thread "
                   f"({dt:.1f}s timed)"),
    }


def main_q17(args):
    """BASELINE config 5 shape at N=1: TPC-H Q17 (two linear joins,
    distinct, per-partkey AVG arrangement, correlated filter, global SUM)
    maintained under lineitem churn; HBM-resident inputs, device-resident
    interior streams (Q17Dataflow.step_dev)."""
    import json as _json

    import torch
    from materialize_amd import _abi as abi
    from materialize_amd._ffi import GpuCtx
    from materialize_amd.tpch import TpchGen
    from materialize_amd.workloads import Q17Dataflow, ShardedQ17Dataflow

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    N = world if world > 1 else 1
    sf = args.sf or (1.0 if N == 1 else 1.25 * N)
    batch_rows = args.batch_rows or 100_000 * N
    ndev = max(torch.cuda.device_count(), 1)
    dev_idx = local_rank % ndev
    device = f"cuda:{dev_idx}"
    torch.cuda.set_device(dev_idx)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group(args.backend)
        from materialize_amd.dist import TorchExchange
        ex = TorchExchange("cpu" if args.backend == "gloo" else device)
    ctx = GpuCtx(device=dev_idx)
    gen = TpchGen(sf=sf, seed=args.seed)
    df = ShardedQ17Dataflow(ctx, ex) if world > 1 else Q17Dataflow(ctx)
    df.load(gen)
    ctx.lib.mz_gpu_sync(ctx.ctx)

    K, W = args.steps, args.warmup
    staged = []
    rows = []
    for i in range(W + K):
        lp_k, lp_v, lp_d = gen.churn(batch_rows)["lineitem_by_part"]
        rows.append(len(lp_k))  # whole-job rows (all ranks' shards)
        if world > 1:
            lp_k, lp_v, lp_d = df._filter_shard(lp_k, lp_v, lp_d)
        n = len(lp_k)
        kt = torch.from_numpy(np.ascontiguousarray(lp_k, np.int64)
                              ).to(device)
        vt = torch.from_numpy(np.ascontiguousarray(lp_v, np.uint8)
                              .reshape(-1)).to(device)
        tt = torch.full((n,), i + 1, dtype=torch.int64, device=device)
        dt = torch.from_numpy(np.ascontiguousarray(lp_d, np.int64)
                              ).to(device)
        staged.append(abi.make_updates_from_torch(kt, vt, tt, dt, i + 1,
                                                  i + 2))
    for i in range(W):
        df.step_dev(staged[i], i + 1)
    ctx.lib.mz_gpu_sync(ctx.ctx)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    ctx.set_kernel_timing(1)
    t0 = time.perf_counter()
    for i in range(W, W + K):
        df.step_dev(staged[i], i + 1)
    ctx.lib.mz_gpu_sync(ctx.ctx)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ctx.set_kernel_timing(0)
    if dist:
        e = torch.tensor([elapsed], device=device
                         if args.backend != "gloo" else "cpu")
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.cpu())
    if args.dump_outputs:
        # step_dev applies its corrections to the maintained result, which
        # is what the caller holds after the last timed step
        ks = sorted(df.result)
        sfx = "" if world == 1 else f"_rank{rank}"
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, f"result_keys{sfx}.npy"),
                np.array(ks, np.float64))
        np.save(os.path.join(args.dump_outputs, f"result_sums{sfx}.npy"),
                np.array([float(df.result[k]) for k in ks], np.float64))
    probe_ms, probe_rows, probe_launches = ctx.probe_stats()
    import ctypes as C
    pairs, batches, alg_bytes = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ctx.lib.mz_gpu_get_probe_stats2.argtypes = [C.c_void_p] + \
        [C.POINTER(C.c_uint64)] * 3
    ctx.lib.mz_gpu_get_probe_stats2(ctx.ctx, C.byref(pairs),
                                    C.byref(batches), C.byref(alg_bytes))
    total_rows = sum(rows[W:])
    achieved = (alg_bytes.value / (probe_ms / 1e3)) if probe_ms > 0 else 0.0
    out = {
        "metric": "input update rows/sec maintained (TPC-H Q17)",
        "value": total_rows / elapsed, "unit": "rows/s", "n_gpus": N,
        "steps": K, "warmup": W, "ms_per_step": elapsed / K * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "int64", "data": "synthetic",
        "config": {"workload": f"tpch_q17_sf{sf:g}_churn{batch_rows}",
                   "sf": sf, "batch_rows": batch_rows,
                   "parallelism": f"shards{N}"},
        "roofline": {"bound": "hbm", "achieved": achieved / 1e9,
                     "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK, "traffic": None},
        "cpu_baseline": (run_cpu_baseline_q17(args.seed, batch_rows, sf=sf)
                         if rank == 0 and N == 1 and args.full
                         and not args.no_cpu_baseline else None),
        "probe_kernel": {"ms_total": probe_ms,
                         "launch_pairs": probe_launches // 2,
                         "alg_bytes": alg_bytes.value},
    }
    if rank == 0:
        print(_json.dumps(out))


def main():
    args = parse_args()
    if args.call_profile:
        # engine-side sub-phase event profiling (mz_gpu_prof_dump)
        os.environ.setdefault("MZ_GPU_PROF", "1")
    if args.workload == "q17":
        main_q17(args)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    N = world if world > 1 else args.gpus
    if args.gpus > 1 and world == 1:
        print("ERROR: launch N>1 via torch.distributed.run", file=sys.stderr)
        sys.exit(2)

    import torch
    from materialize_amd import _abi as abi  # noqa: F401
    from materialize_amd._ffi import GpuCtx
    from materialize_amd.tpch import TpchGen
    from materialize_amd.workloads import Q3Dataflow, ShardedQ3Dataflow

    sf = args.sf or (1.0 if N == 1 else 1.25 * N)
    batch_rows = args.batch_rows or 100_000 * N
    ndev = max(torch.cuda.device_count(), 1)
    dev_idx = local_rank % ndev  # gloo validation: several ranks, one GPU
    device = f"cuda:{dev_idx}"
    torch.cuda.set_device(dev_idx)

    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group(args.backend)
        from materialize_amd.dist import TorchExchange
        ex = TorchExchange("cpu" if args.backend == "gloo" else device)
    ctx = GpuCtx(device=dev_idx)

    gen = TpchGen(sf=sf, seed=args.seed)
    if world > 1:
        df = ShardedQ3Dataflow(ctx, ex)
    else:
        df = Q3Dataflow(ctx)
    df.load(gen)
    df.maintain()
    ctx.lib.mz_gpu_sync(ctx.ctx)

    # pre-generate + pre-filter + pre-stage all churn batches (untimed).
    # One extra batch beyond the window: the 1-deep insert pipeline means
    # step i also enqueues batch i+1's lane consolidations, so the timed
    # region executes exactly K ingest pipelines (batches W+1..W+K; batch
    # W's ran during warmup, priming the pipeline) — the closing
    # mz_gpu_sync waits for the lanes, keeping the window honest.
    K, W = args.steps, args.warmup
    pipeline = not args.no_pipeline
    staged = []
    rows_per_step = []
    for i in range(W + K + (1 if pipeline else 0)):
        churn = gen.churn(batch_rows)
        if i < W + K:
            rows_per_step.append(len(churn["lineitem"][0]) +
                                 len(churn["orders"][0]))
        churn = filter_shard(churn, world, rank)
        staged.append(stage_churn(churn, i + 1, device))

    def nxt(i):
        return staged[i + 1] if pipeline and i + 1 < len(staged) else None

    for i in range(W):
        corr = df.step_dev(staged[i], i + 1, next_upd=nxt(i))
        if corr is not None:
            corr.release()
    # device-wide sync WITHOUT mz_gpu_sync: that call force-flushes
    # pending inserts, which would install batch W before the window and
    # break the primed 1-deep pipeline (the closing sync below still
    # installs/drains everything inside the timed region)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()

    prof = CallProfiler(ctx) if args.call_profile else None
    if prof:
        print("# MZPROF setup+warmup (discard):", file=sys.stderr)
        ctx.prof_dump()  # reset engine sub-phase counters before timing
    ctx.set_kernel_timing(1)
    step_times = [] if os.environ.get("MZ_BENCH_STEP_TIMES") else None
    # --dump-outputs keeps the last timed step's corrections alive past
    # the window (released after the copy-out below)
    keep = W + K - 1 if args.dump_outputs else -1
    last_corr = None
    t0 = time.perf_counter()
    for i in range(W, W + K):
        corr = df.step_dev(staged[i], i + 1, next_upd=nxt(i))
        if corr is not None:
            if i == keep:
                last_corr = corr
            else:
                corr.release()
        if step_times is not None:
            torch.cuda.synchronize()  # not mz_gpu_sync: keep pendings
            step_times.append(time.perf_counter() - t0 -
                              sum(step_times))
    ctx.lib.mz_gpu_sync(ctx.ctx)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if step_times is not None:
        print("# step_ms " + " ".join(f"{s*1e3:.1f}" for s in step_times),
              file=sys.stderr)
    ctx.set_kernel_timing(0)
    if args.dump_outputs:
        cols = last_corr.to_host() if last_corr is not None else None
        if last_corr is not None:
            last_corr.release()
        dump_outputs(args.dump_outputs, cols, rank, world)
    if prof:
        print(f"# step wall {elapsed/K*1e3:.2f} ms; breakdown:",
              file=sys.stderr)
        prof.report(K)
        ctx.prof_dump()  # MZPROF sub-phase lines (stderr)

    if dist:
        e = torch.tensor([elapsed], device=device)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.cpu())

    probe_ms, probe_rows, probe_launches = ctx.probe_stats()
    import ctypes as C
    pairs, batches, alg_bytes = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ctx.lib.mz_gpu_get_probe_stats2.argtypes = [C.c_void_p] + \
        [C.POINTER(C.c_uint64)] * 3
    ctx.lib.mz_gpu_get_probe_stats2(ctx.ctx, C.byref(pairs),
                                    C.byref(batches), C.byref(alg_bytes))

    total_rows = sum(rows_per_step[W:])
    value = total_rows / elapsed
    achieved = (alg_bytes.value / (probe_ms / 1e3)) if probe_ms > 0 else 0.0
    roofline = {
        "bound": "hbm",
        "achieved": achieved,
        "peak": HBM_PEAK,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK,
        "traffic": None,
    }
    # normalize achieved/peak into GB/s for the printed unit
    roofline["achieved"] = achieved / 1e9
    roofline["peak"] = HBM_PEAK / 1e9
    # measured HBM traffic per probe launch-pair (separate PMC passes; see
    # profiles/traffic_*.json for provenance) when this exact workload was
    # the one profiled
    try:
        import glob as _glob
        for tf in sorted(_glob.glob(os.path.join(REPO, "profiles",
                                                 "traffic_*.json"))):
            td = json.load(open(tf))
            if td.get("workload") == (f"tpch_q3_sf{sf:g}_churn{batch_rows}"
                                      if N == 1 else None):
                roofline["traffic"] =                     td["probe_pair_traffic_bytes_per_launch"]
    except Exception:
        pass

    cpu_baseline = None
    if rank == 0 and N == 1 and args.full and not args.no_cpu_baseline:
        # same batch size as the GPU run (bounded step count)
        bsteps = 4 if batch_rows <= 200_000 else 2
        cpu_baseline = run_cpu_baseline(args.seed, batch=batch_rows,
                                        steps=bsteps, sf=sf)

    if rank == 0:
        line = {
            "metric": METRIC,
            "value": value,
            "unit": "rows/s",
            "n_gpus": N,
            "steps": K,
            "warmup": W,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int64",
            "data": "synthetic",
            "config": {
                "workload": (f"tpch_q3_sf{sf:g}_churn{batch_rows}" +
                             ("" if N == 1 else f"_shards{N}")),
                "sf": sf,
                "batch_rows": batch_rows,
                "parallelism": f"shards{N}",
            },
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
            "probe_kernel": {
                "ms_total": probe_ms,
                "delta_rows": probe_rows,
                "emitted_pairs": pairs.value,
                "launch_pairs": probe_launches // 2,
                "alg_bytes": alg_bytes.value,
            },
        }
        print(json.dumps(line))
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
