"""Spine maintenance policy on the GPU: the pair rule and its cascades,
the small-batch pool, the hard cap, deferred merges, flush_take under a
small policy, and dropping an arrangement that used the cached sort plan.

The policy knobs (MZ_GPU_SMALL, MZ_GPU_SMALL_POOL, MZ_GPU_GEO,
MZ_GPU_DEFER_MERGE) are read once per process, so every configuration runs
its body in a fresh child process: this file run as a script with the case
name. The child checks the arrangement against the oracle after every
insert (identity half-join of present keys, byte-equal) and prints one
`RESULT {json}` line that the parent test asserts on.

Every inserted row has a fresh key, diff +1 and time t, so consolidation
removes nothing and batch sizes are exactly the insert sizes.
"""
import json
import os
import subprocess
import sys
from itertools import accumulate

import numpy as np
import pytest

gpu = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [3000, 3000, 3000, 3000, 1000, 1000, 1000, 500, 2000, 2500, 6000,
         1, 700]
SMALL_ENV = {"MZ_GPU_SMALL": "4096", "MZ_GPU_SMALL_POOL": "2"}
SYNC_N_BATCHES = [1, 1, 2, 1, 2, 3, 2, 3, 2, 3, 1, 2, 3]
CAP_SIZES = [100] * 13
CAP_N_BATCHES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 2, 3]


def model_n_batches(sizes, small, pool, geo=1.0, cap=10):
    """The synchronous policy restated over batch sizes: after each push,
    the pair rule until it rests, the pool rule once, then the cap."""
    b, out = [], []
    for n in sizes:
        b.append(n)
        while len(b) >= 2 and b[-2] <= geo * b[-1] and b[-2] + b[-1] >= small:
            b[-2:] = [b[-2] + b[-1]]
        i = len(b)
        while i > 0 and b[i - 1] < small:
            i -= 1
        if len(b) - i > pool:
            b[i:] = [sum(b[i:])]
        if len(b) > cap:
            b[:] = [sum(b)]
        out.append(len(b))
    return out


def test_model_gives_the_expected_sequences():
    assert model_n_batches(SIZES, 4096, 2) == SYNC_N_BATCHES
    assert model_n_batches(SIZES[:4], 4096, 2) == SYNC_N_BATCHES[:4]
    assert model_n_batches(CAP_SIZES, 4 << 20, 20) == CAP_N_BATCHES


def run_child(case, env_extra):
    env = dict(os.environ)
    for k in ("MZ_GPU_SMALL", "MZ_GPU_SMALL_POOL", "MZ_GPU_GEO",
              "MZ_GPU_DEFER_MERGE"):
        env.pop(k, None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), case],
                       env=env, timeout=120, check=True,
                       stdout=subprocess.PIPE, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0][len("RESULT "):])


@gpu
def test_sync_policy_pair_cascades_and_pool():
    r = run_child("sync", SMALL_ENV)
    assert SYNC_N_BATCHES == model_n_batches(SIZES, 4096, 2)
    assert r["n_batches"] == SYNC_N_BATCHES
    assert r["n_updates"] == list(accumulate(SIZES))
    assert r["parity_checks"] == len(SIZES)


@gpu
def test_hard_cap():
    r = run_child("cap", {"MZ_GPU_SMALL_POOL": "20"})
    assert CAP_N_BATCHES == model_n_batches(CAP_SIZES, 4 << 20, 20)
    assert r["n_batches"] == CAP_N_BATCHES
    assert r["n_updates"] == list(accumulate(CAP_SIZES))
    assert r["parity_checks"] == len(CAP_SIZES)


@gpu
def test_deferred_merges():
    r = run_child("deferred", dict(SMALL_ENV, MZ_GPU_DEFER_MERGE="1"))
    assert r["parity_checks"] == len(SIZES) + 1
    assert r["n_updates_after_sync"] == sum(SIZES)
    assert r["n_batches_after_maintain"] == 1
    assert r["n_updates_after_maintain"] == sum(SIZES)


@gpu
def test_flush_take_under_small_policy():
    r = run_child("flush_take", SMALL_ENV)
    assert r["taken_rows"] == [3000] * 4
    assert r["n_batches"] == model_n_batches([3000] * 4, 4096, 2)
    assert r["n_updates"] == [3000, 6000, 9000, 12000]
    assert r["parity_checks"] == 4


@gpu
def test_drop_after_cached_plan():
    """Two device-staged inserts (the second sorts with the cached plan),
    drop, sync; the context then serves a new arrangement."""
    from materialize_amd._ffi import GpuCtx
    from pyoracle import OracleCtx
    g, o = GpuCtx(), OracleCtx()
    a = g.arr_create(SCH())
    rng = np.random.default_rng(7)
    keep = []
    for t in range(2):
        # interleaved fresh keys: the second batch's column ranges lie
        # inside the first's, so its sort reuses the cached plan
        k, v = fresh_rows(rng, 0, 8000, shuffle=True)
        k, v = k[k % 2 == t], v[k % 2 == t]
        keep.append(insert_dev(g, a, k, v, t))
        g.arr_flush(a)
    g.lib.mz_gpu_arr_drop(g.ctx, a)
    g.lib.mz_gpu_sync(g.ctx)
    ga, oa = g.arr_create(SCH()), o.arr_create(SCH())
    k, v = fresh_rows(rng, 0, 3000)
    g.arr_insert(ga, host_updates(k, v, 2))
    o.arr_insert(oa, host_updates(k, v, 2))
    check_parity(g, o, ga, oa, rng, 3000, 2)
    assert g.arr_stats(ga)[1] == 3000
    g.close()
    o.close()


# ------------------------------------------------- shared with the child

def SCH():
    from materialize_amd import _abi as abi
    return abi.schema(1, 8)


def fresh_rows(rng, first_key, n, shuffle=False):
    keys = np.arange(first_key, first_key + n, dtype=np.int64)
    if shuffle:
        rng.shuffle(keys)
    vals = rng.integers(-2**40, 2**40, n).astype(np.int64) \
        .reshape(-1, 1).view(np.uint8).reshape(n, 8)
    return keys, vals


def host_updates(keys, vals, t):
    from materialize_amd import _abi as abi
    n = len(keys)
    return abi.make_updates(keys, vals, np.full(n, t, np.uint64),
                            np.ones(n, np.int64), t, t + 1)


def insert_dev(g, arr, keys, vals, t):
    """Device-staged arr_insert_async; returns the tensors, which must
    outlive the flush."""
    import torch
    from materialize_amd._abi import make_updates_from_torch
    n = len(keys)
    refs = (torch.from_numpy(np.ascontiguousarray(keys)).cuda(),
            torch.from_numpy(np.ascontiguousarray(vals).reshape(-1)).cuda(),
            torch.full((n,), t, dtype=torch.int64).cuda(),
            torch.ones(n, dtype=torch.int64).cuda())
    g.arr_insert_async(arr, make_updates_from_torch(*refs, t, t + 1))
    return refs


def check_parity(g, o, ga, oa, rng, n_keys, t):
    """Identity half-join of a few hundred present keys at time t against
    the oracle, byte-equal."""
    from materialize_amd import _abi as abi
    cl = abi.closure([], [abi.field(abi.MZ_SRC_KEY, 0, 8)],
                     [abi.field(abi.MZ_SRC_VAL_LOOKUP, 0, 8)],
                     abi.schema(1, 8))
    pk = np.unique(rng.integers(0, n_keys, 300)).astype(np.int64)
    pk = np.union1d(pk, [0, n_keys - 1]).astype(np.int64)
    pu = abi.make_updates(pk, None, np.full(len(pk), t, np.uint64),
                          np.ones(len(pk), np.int64), t, t + 1)
    rg = g.halfjoin(ga, pu, 0, True, cl)
    ro = o.halfjoin(oa, pu, 0, True, cl)
    assert len(ro[2]) == len(pk)
    for x, y, what in zip(rg, ro, ("keys", "vals", "times", "diffs")):
        np.testing.assert_array_equal(np.asarray(x).view(np.uint8),
                                      np.asarray(y).view(np.uint8),
                                      err_msg=f"{what} at t={t}")


def child(case):
    # torch first, as under pytest and in bench.py: the device-staged
    # inserts need the library and torch on one HIP runtime, torch's
    import torch
    assert torch.cuda.is_available()
    from materialize_amd._ffi import GpuCtx
    from pyoracle import OracleCtx
    g, o = GpuCtx(), OracleCtx()
    ga, oa = g.arr_create(SCH()), o.arr_create(SCH())
    rng = np.random.default_rng(11)
    sizes = {"sync": SIZES, "deferred": SIZES, "cap": CAP_SIZES,
             "flush_take": [3000] * 4}[case]
    res = {"n_batches": [], "n_updates": [], "taken_rows": [],
           "parity_checks": 0}
    total, keep = 0, []
    for t, n in enumerate(sizes):
        keys, vals = fresh_rows(rng, total, n, shuffle=True)
        u = host_updates(keys, vals, t)
        if case == "flush_take":
            keep.append(insert_dev(g, ga, keys, vals, t))
            took = g.arr_flush_take(ga)
            want = o.consolidate(SCH(), u)
            for x, y, what in zip(took.to_host(), want,
                                  ("keys", "vals", "times", "diffs")):
                np.testing.assert_array_equal(
                    np.asarray(x).view(np.uint8),
                    np.asarray(y).view(np.uint8),
                    err_msg=f"taken {what} at t={t}")
            res["taken_rows"].append(took.n)
            took.release()
        else:
            g.arr_insert(ga, u)
        o.arr_insert(oa, u)
        total += n
        check_parity(g, o, ga, oa, rng, total, t)
        res["parity_checks"] += 1
        if case != "deferred":  # installs there depend on an event query
            nb, nu, _ = g.arr_stats(ga)
            res["n_batches"].append(nb)
            res["n_updates"].append(nu)
    if case == "deferred":
        g.lib.mz_gpu_sync(g.ctx)
        res["n_updates_after_sync"] = g.arr_stats(ga)[1]
        g.arr_maintain(ga)
        nb, nu, _ = g.arr_stats(ga)
        res["n_batches_after_maintain"] = nb
        res["n_updates_after_maintain"] = nu
        check_parity(g, o, ga, oa, rng, total, len(sizes))
        res["parity_checks"] += 1
    g.close()
    o.close()
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    for p in (REPO, os.path.join(REPO, "oracle")):
        sys.path.insert(0, p)
    child(sys.argv[1])
