"""Cost of a full-scan peek ("Full-scan peek").

One arrangement of 1-word keys and 16-byte vals is built from --batches
device-resident inserts of --rows random rows each (times 0, 1, ...), then
read back whole two ways, as of each time in --as-of:

  scan   mz_gpu_peek_scan with the identity closure
  keyed  mz_gpu_peek over all distinct keys — the only way to read
         everything before the scan existed; its key list is host memory,
         as that entry requires

Per way: the median host-clock time of --calls calls after --warmup (each
call ends in the engine's own closing device synchronize; out-batches are
released without copying them to the host), and, from a second loop with
kernel timing on, the probe kernel's device-event time (k_scan_walk or
k_probe_walk alone, without the consolidation that follows) with the
algorithmic bytes the drivers model and the resulting GB/s. Prints one JSON
line. Needs a GPU: there is no fallback.

    python profiles/peek_scan_cost.py [--rows 1000000] [--batches 6]
"""
import argparse
import ctypes as C
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
    p.add_argument("--batches", type=int, default=6)
    p.add_argument("--keys", type=int, default=2_000_000)
    p.add_argument("--as-of", type=int, nargs="+", default=None)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--seed", type=int, default=11)
    args = p.parse_args()

    import numpy as np
    import torch
    from materialize_amd import _abi as abi
    from materialize_amd._ffi import GpuCtx

    if not torch.cuda.is_available():
        raise SystemExit("peek_scan_cost: no GPU")
    dev = torch.device("cuda:0")
    g = GpuCtx()
    lib = g.lib
    lib.mz_gpu_get_probe_stats2.argtypes = [C.c_void_p] + \
        [C.POINTER(C.c_uint64)] * 3
    arr = g.arr_create(abi.schema(1, 16))
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    n = args.rows
    diffs = torch.ones(n, dtype=torch.int64, device=dev)
    seen = []
    for t in range(args.batches):
        keys = torch.randint(0, args.keys, (n,), dtype=torch.int64,
                             device=dev, generator=gen)
        vals = torch.randint(-2**62, 2**62, (n, 2), dtype=torch.int64,
                             device=dev, generator=gen)
        times = torch.full((n,), t, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        g.arr_insert(arr, abi.make_updates_from_torch(
            keys, vals.view(torch.uint8).reshape(-1), times, diffs, t, t + 1))
        seen.append(keys.cpu().numpy())
    allkeys = np.unique(np.concatenate(seen)).astype(np.int64)
    kptr = allkeys.view(np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    n_batches, n_updates, hbm_bytes = g.arr_stats(arr)

    def scan(as_of):
        out = g.peek_scan_dev(arr, as_of)
        rows = out.n
        out.release()
        return rows

    def keyed(as_of):
        outp = C.POINTER(abi.OutBatch)()
        g._check(lib.mz_gpu_peek(g.ctx, arr, kptr, len(allkeys), as_of,
                                 C.byref(outp)))
        rows = int(outp.contents.n)
        lib.mz_gpu_out_release(g.ctx, outp)
        return rows

    def measure(call, as_of):
        for _ in range(args.warmup):
            rows = call(as_of)
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call(as_of)
            ms.append((time.perf_counter() - t0) * 1e3)
        # the probe kernel alone, from the events run_probe records
        g.set_kernel_timing(True)
        g.probe_stats()
        pairs, batches, alg = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib.mz_gpu_get_probe_stats2(g.ctx, C.byref(pairs), C.byref(batches),
                                    C.byref(alg))
        kms, kbytes, nlaunch = [], [], 0
        for _ in range(args.calls):
            call(as_of)
            k, _rows, launches = g.probe_stats()
            lib.mz_gpu_get_probe_stats2(g.ctx, C.byref(pairs),
                                        C.byref(batches), C.byref(alg))
            nlaunch = max(nlaunch, launches)
            kms.append(k)
            kbytes.append(alg.value)
        g.set_kernel_timing(False)
        kmed = statistics.median(kms)
        return {"out_rows": rows,
                "call_median_ms": round(statistics.median(ms), 3),
                "call_min_ms": round(min(ms), 3),
                "call_max_ms": round(max(ms), 3),
                "kernel_median_ms": round(kmed, 4),
                "kernel_min_ms": round(min(kms), 4),
                "kernel_max_ms": round(max(kms), 4),
                "kernel_launches_max": nlaunch,
                "alg_bytes": kbytes[0],
                "alg_GBps": round(kbytes[0] / kmed / 1e6, 1)}

    res = {"rows_per_batch": n, "inserts": args.batches,
           "spine_batches": n_batches, "updates": n_updates,
           "arr_hbm_bytes": hbm_bytes, "distinct_keys": len(allkeys),
           "warmup": args.warmup, "calls": args.calls, "as_of": {}}
    for as_of in (args.as_of or [args.batches - 1]):
        s, k = measure(scan, as_of), measure(keyed, as_of)
        assert s["out_rows"] == k["out_rows"]
        res["as_of"][str(as_of)] = {
            "scan": s, "keyed": k,
            "call_ratio_keyed_over_scan":
                round(k["call_median_ms"] / s["call_median_ms"], 2),
            "kernel_ratio_keyed_over_scan":
                round(k["kernel_median_ms"] / s["kernel_median_ms"], 2)}
    print(json.dumps(res))
    g.close()


if __name__ == "__main__":
    main()
