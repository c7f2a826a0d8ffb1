"""Cost of a scalar-expression MFP call ("Scalar-expression
MFP").

Device-resident streams of (key, [a, b]) rows, keys in [-100, 100), a and b in
[0, 50), one timestamp per third of the rows, diffs +-1. Per --rows point:

 (a) tests/test_map.py's closure (filter a > 10; re-key to b; out val = (old
     key, a)) through mz_gpu_map and, as an expression program, through
     mz_gpu_mfp(consolidate = 0): the two alternate in one process, --calls
     calls each after 2 warm-up calls each, host clock around the call (both
     end in the engine's own synchronisation; the out-batches are released
     without copying them to the host).
 (b) a 31-op program through mz_gpu_mfp(consolidate = 0): FILTER a + b > 5;
     FILTER a * 2 < 90; OUT key; OUT IF(b = 0, NULL, a / b) nullable;
     OUT a - b; OUT a % 7.

For both programs, from --calls more calls with kernel timing on, the
device-event time of k_mfp_eval alone and the bytes/s it achieves over the
algorithmic bytes: 8 kw + vb + 16 in per row, 8 okw + ovb + 16 out per
emitted row. Prints one JSON line. Needs a GPU: there is no fallback.

    python profiles/mfp_cost.py [--rows 1000000 4000000] [--calls 8]
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
    p.add_argument("--rows", type=int, nargs="+",
                   default=[1_000_000, 4_000_000])
    p.add_argument("--calls", type=int, default=8)
    p.add_argument("--seed", type=int, default=11)
    args = p.parse_args()

    import torch
    from materialize_amd import _abi as abi
    from materialize_amd._ffi import GpuCtx

    if not torch.cuda.is_available():
        raise SystemExit("mfp_cost: no GPU")
    dev = torch.device("cuda:0")
    g = GpuCtx()
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    KEY, VS = abi.MZ_SRC_KEY, abi.MZ_SRC_VAL_STREAM
    sch = abi.schema(1, 16)
    key, a, b = abi.x_col(KEY, 0), abi.x_col(VS, 0), abi.x_col(VS, 8)
    cl = abi.closure(
        [abi.filt(VS, 0, 8, abi.MZ_CMP_GT, 10)], [abi.field(VS, 8, 8)],
        [abi.field(KEY, 0, 8), abi.field(VS, 0, 8)], sch)
    rekey = abi.mfp_spec(sch, sch, [
        abi.x_filter(a > 10), abi.x_out_key(b, 0),
        abi.x_out_val(key, 0, 8), abi.x_out_val(a, 8, 8)])
    out_b = abi.schema(1, 25)
    prog = abi.mfp_spec(sch, out_b, [
        abi.x_filter(a + b > 5), abi.x_filter(a * 2 < 90),
        abi.x_out_key(key, 0),
        abi.x_out_val(abi.x_if(b == 0, abi.x_null("int"), a // b), 0, 8,
                      nullable=1),
        abi.x_out_val(a - b, 9, 8), abi.x_out_val(a % 7, 17, 8)])

    def stats(ms, what, nd=3):
        return {f"{what}_median_ms": round(statistics.median(ms), nd),
                f"{what}_min_ms": round(min(ms), nd),
                f"{what}_max_ms": round(max(ms), nd)}

    def point(n):
        keys = torch.randint(-100, 100, (n,), dtype=torch.int64, device=dev,
                             generator=gen)
        vals = torch.randint(0, 50, (n, 2), dtype=torch.int64, device=dev,
                             generator=gen)
        times = torch.arange(n, dtype=torch.int64, device=dev) % 3
        diffs = torch.randint(0, 2, (n,), dtype=torch.int64, device=dev,
                              generator=gen) * 2 - 1
        torch.cuda.synchronize()
        u = abi.make_updates_from_torch(
            keys, vals.view(torch.uint8).reshape(-1), times, diffs, 0, 3)

        def call_map():
            outp = C.POINTER(abi.OutBatch)()
            t0 = time.perf_counter()
            g._check(g.lib.mz_gpu_map(g.ctx, C.byref(sch), C.byref(u),
                                      C.byref(cl), C.byref(outp)))
            ms = (time.perf_counter() - t0) * 1e3
            rows = int(outp.contents.n)
            g.lib.mz_gpu_out_release(g.ctx, outp)
            return ms, rows

        def call_mfp(spec):
            t0 = time.perf_counter()
            out = g.mfp_dev(spec, u, consolidate=False)
            ms = (time.perf_counter() - t0) * 1e3
            rows = out.n
            out.release()
            return ms, rows

        for _ in range(2):
            call_map(), call_mfp(rekey), call_mfp(prog)
        ms_map, ms_mfp, ms_prog = [], [], []
        for _ in range(args.calls):  # alternating
            ms_map.append(call_map()[0])
            ms_mfp.append(call_mfp(rekey)[0])
            ms_prog.append(call_mfp(prog)[0])
        rows_map = call_map()[1]

        def kernel(spec, osch):
            g.set_kernel_timing(True)
            g.probe_stats()
            kms = []
            for _ in range(args.calls):
                _, rows = call_mfp(spec)
                kms.append(g.probe_stats()[0])
            g.set_kernel_timing(False)
            nbytes = n * (8 * 1 + 16 + 16) + rows * (
                8 * osch.key_words + osch.val_bytes + 16)
            med = statistics.median(kms)
            return rows, dict(stats(kms, "eval_kernel", 4),
                              alg_bytes=nbytes,
                              eval_kernel_gb_per_s=round(
                                  nbytes / (med * 1e-3) / 1e9, 1))

        rows_a, ka = kernel(rekey, sch)
        rows_b, kb = kernel(prog, out_b)
        assert rows_a == rows_map
        return {"rows": n,
                "rekey": dict(stats(ms_map, "map_call"),
                              **stats(ms_mfp, "mfp_call"), out_rows=rows_a,
                              n_ops=rekey.n_ops, **ka),
                "program": dict(stats(ms_prog, "mfp_call"), out_rows=rows_b,
                                n_ops=prog.n_ops, **kb)}

    res = {"calls": args.calls, "points": [point(n) for n in args.rows]}
    print(json.dumps(res))
    g.close()


if __name__ == "__main__":
    main()
