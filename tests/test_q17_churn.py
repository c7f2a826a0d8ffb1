"""Q17 maintained on a tiny universe, checked after every step against a
plain-Python recompute over explicit state.

`Q17Dataflow._push` is driven directly with hand-built columns: a handful
of partkeys, lineitem deltas that retract and insert, and part deltas that
move a partkey into or out of the (brand, container) match set in the
same step as lineitem deltas for that partkey. Beside the maintained
result, the per-partkey average state (`arr_avg`) and the distinct set
(`arr_dist`) are peeked and held to the reference's exact (sum, count)
and membership at multiplicity 1: the filter `5*q*count < sum` does not
see a uniform scale of sum and count, the interior state does.

Everything compared is integers; every check is exact equality."""
import functools
from collections import Counter

import numpy as np
import pytest

from materialize_amd import _abi as abi
from materialize_amd.tpch import TpchGen
from materialize_amd.workloads import Q17Dataflow

BRAND, CONTAINER = 23, 10          # the match set of q17_closures
PARTKEYS = list(range(1, 9))
PEEK_KEYS = PARTKEYS + [9]         # 9 never exists
PK_WEIGHTS = [.25, .25, .15, .15, .05, .05, .05, .05]
SEED = 106   # meets reference()'s input conditions, part idle or not


class RefQ17:
    """Q17 recomputed from scratch over explicit state: `items` is the
    multiset {(partkey, quantity, extendedprice): multiplicity} of
    lineitems, `parts` maps partkey -> (brand, container)."""

    def __init__(self):
        self.items = Counter()
        self.parts = {}

    def apply(self, lp_rows, part_rows):
        """lp_rows: (partkey, quantity, extendedprice, diff); part_rows:
        (partkey, brand, container, diff), retractions first."""
        for pk, q, ep, d in lp_rows:
            self.items[(pk, q, ep)] += d
            assert self.items[(pk, q, ep)] >= 0
        self.items = +self.items
        for pk, b, c, d in part_rows:
            if d < 0:
                assert self.parts.pop(pk) == (b, c)
            else:
                assert d == 1 and pk not in self.parts
                self.parts[pk] = (b, c)

    def matches(self, pk):
        return self.parts.get(pk) == (BRAND, CONTAINER)

    def stats(self):
        """{partkey: (sum(quantity), count)} over ALL lineitems of each
        partkey in the distinct set: the matching parts that have at
        least one lineitem."""
        st = {}
        for (pk, q, _), m in self.items.items():
            if self.matches(pk):
                s, c = st.get(pk, (0, 0))
                st[pk] = (s + q * m, c + m)
        return st

    def qualifying(self):
        """The surviving rows (lineitems of matching parts) that pass
        quantity < 0.2 * avg, in the exact integer form."""
        st = self.stats()
        return {r for r in self.items
                if r[0] in st and 5 * r[1] * st[r[0]][1] < st[r[0]][0]}

    def result(self):
        """sum(extendedprice) over the qualifying rows; None when no row
        qualifies (the global SUM then has no group)."""
        rows = self.qualifying()
        if not rows:
            return None
        return sum(r[2] * self.items[r] for r in rows)


def _part(pk, brand, container, d):
    return (pk, brand, container, d)


def deterministic_steps():
    """Both parts match throughout. t1 makes pk1's four small rows
    qualify; t2 brings pk2 into the distinct set in the same step as its
    lineitem delta; t3 retracts it again; t4 re-enters pk2 over state
    that must have been fully retracted. Results: None, 1000, 1007,
    1000, 1000."""
    return [
        ([(1, 1, 100, 1), (1, 1, 200, 1), (1, 1, 300, 1), (1, 1, 400, 1)],
         [_part(1, BRAND, CONTAINER, 1), _part(2, BRAND, CONTAINER, 1)]),
        ([(1, 30, 5000, 1)], []),
        ([(2, 1, 7, 1), (2, 40, 9, 1)], []),
        ([(2, 1, 7, -1), (2, 40, 9, -1)], []),
        ([(2, 10, 7, 1), (2, 40, 9, 1)], []),
    ]


DETERMINISTIC_WANT = [None, 1000, 1007, 1000, 1000]


def random_steps(seed, nsteps=12):
    """8 partkeys, brand in {23, 5}, container in {10, 3}, quantities in
    1..50. Every step retracts some existing lineitems and inserts new
    ones; every third step also retracts a part row and inserts it with
    the other brand, together with a lineitem insert for that partkey."""
    rng = np.random.default_rng(seed)
    ref = RefQ17()
    steps = []
    for t in range(nsteps):
        lp, part = [], []
        if t == 0:
            part = [_part(pk, int(rng.choice([BRAND, 5])),
                          int(rng.choice([CONTAINER, 3])), 1)
                    for pk in PARTKEYS]
        live = sorted(ref.items)
        n_ret = min(len(live), int(rng.integers(2, 9))) if t else 0
        if n_ret:
            for i in rng.choice(len(live), n_ret, replace=False):
                row = live[int(i)]
                lp.append(row + (-int(rng.integers(1, ref.items[row] + 1)),))
        # skewed partkeys: the rare ones run empty and come back, so the
        # distinct set also moves through lineitem churn alone
        for _ in range(32 if t == 0 else int(rng.integers(2, 9))):
            lp.append((int(rng.choice(PARTKEYS, p=PK_WEIGHTS)),
                       int(rng.integers(1, 51)),
                       int(rng.integers(1, 1000)), int(rng.integers(1, 3))))
        if t and t % 3 == 0:
            # flip a part that can match (container 10) when there is one,
            # so the partkey enters or leaves the match set
            cand = [pk for pk in PARTKEYS if ref.parts[pk][1] == CONTAINER]
            pk = int(rng.choice(cand or PARTKEYS))
            b, c = ref.parts[pk]
            part = [_part(pk, b, c, -1),
                    _part(pk, 5 if b == BRAND else BRAND, c, 1)]
            lp.append((pk, int(rng.integers(1, 51)),
                       int(rng.integers(1, 1000)), 1))
        ref.apply(lp, part)
        steps.append((lp, part))
    return steps


def lineitem_only(steps):
    """The same lineitem deltas with the part input idle after t0."""
    return [steps[0]] + [(lp, []) for lp, _ in steps[1:]]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(steps, per-step (result, stats)) of a scenario, computed once and
    shared read-only; checks on the reference alone that the scenario
    holds what the cases are about."""
    steps = {"deterministic": deterministic_steps,
             "random": lambda: random_steps(SEED),
             "deterministic-lineitem": lambda: lineitem_only(
                 deterministic_steps()),
             "random-lineitem": lambda: lineitem_only(random_steps(SEED)),
             }[name]()
    ref = RefQ17()
    want, quals, surv = [], [], []
    for lp, part in steps:
        ref.apply(lp, part)
        want.append((ref.result(), ref.stats()))
        quals.append(ref.qualifying())
        surv.append({r for r in ref.items if ref.matches(r[0])})
    if name == "deterministic":
        assert [w[0] for w in want] == DETERMINISTIC_WANT
    if name.startswith("random"):
        assert 2 * sum(w[0] is not None for w in want) >= len(want), \
            "bad seed: result mostly empty"
        flips = enters = leaves = 0
        for i in range(1, len(want)):
            both = surv[i - 1] & surv[i]
            flips += bool(both & (quals[i - 1] ^ quals[i]))
            enters += len(set(want[i][1]) - set(want[i - 1][1]))
            leaves += len(set(want[i - 1][1]) - set(want[i][1]))
        assert flips, "bad seed: no surviving row's filter outcome flips"
        assert enters >= 2 and leaves >= 2, "bad seed: distinct set static"
    if name == "random":
        # a partkey moves into or out of the match set in the same step
        # as a lineitem delta for it (random_steps builds this in)
        assert any(part and t and {r[0] for r in part} & {r[0] for r in lp}
                   for t, (lp, part) in enumerate(steps))
    return steps, want


def lp_cols(rows):
    k = np.array([r[0] for r in rows], np.int64)
    q = np.array([r[1] for r in rows], np.int64)
    ep = np.array([r[2] for r in rows], np.int64)
    d = np.array([r[3] for r in rows], np.int64)
    return k, TpchGen.lineitem_bypart_vals(q, ep), d


def part_cols(rows):
    """part val, as TpchGen.part_updates: [brand i64][container i64]."""
    n = len(rows)
    k = np.array([r[0] for r in rows], np.int64)
    v = np.zeros((n, 16), np.uint8)
    v[:, 0:8] = np.array([r[1] for r in rows], np.int64).view(
        np.uint8).reshape(n, 8)
    v[:, 8:16] = np.array([r[2] for r in rows], np.int64).view(
        np.uint8).reshape(n, 8)
    return k, v, np.array([r[3] for r in rows], np.int64)


def push(df, t, lp, part):
    df._push(t, lp_cols(lp), part_cols(part) if part else None)


def _i128(b):
    return int.from_bytes(bytes(b), "little", signed=True)


def check_state(df, t, want, what=""):
    """Maintained result and interior state against the reference."""
    result, stats = want
    assert df.result.get(0) == result, f"{what}t{t}: result"
    ctx = df.ctx
    # arr_avg: one row of multiplicity 1 per member of the distinct set;
    # 24-byte aggregate slots, value at +8: SUM i128, then COUNT
    k, v, _, d = ctx.peek(df.arr_avg, PEEK_KEYS, t)
    v = np.asarray(v).reshape(len(k), 48)
    got = [(int(k[i]), _i128(v[i][8:24]), _i128(v[i][32:48]), int(d[i]))
           for i in range(len(k))]
    assert sorted(got) == sorted((pk, s, c, 1)
                                 for pk, (s, c) in stats.items()), \
        f"{what}t{t}: arr_avg (partkey, sum, count, multiplicity)"
    k, _, _, d = ctx.peek(df.arr_dist, PEEK_KEYS, t)
    assert sorted(zip(k.tolist(), d.tolist())) == \
        sorted((pk, 1) for pk in stats), f"{what}t{t}: arr_dist"


def run_push(ctx, name, what=""):
    steps, want = reference(name)
    df = Q17Dataflow(ctx)
    results = []
    for t, (lp, part) in enumerate(steps):
        push(df, t, lp, part)
        check_state(df, t, want[t], what)
        results.append(dict(df.result))
    return results


def test_q17_deterministic_oracle():
    from pyoracle import OracleCtx
    ctx = OracleCtx()
    run_push(ctx, "deterministic")
    ctx.close()


def test_q17_random_churn_oracle():
    from pyoracle import OracleCtx
    ctx = OracleCtx()
    run_push(ctx, "random")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deterministic", "random"])
def test_q17_push_gpu(name):
    """Both scenarios through `_push` on the engine: against the
    reference (result and interior state) and against the oracle."""
    from materialize_amd._ffi import GpuCtx
    from pyoracle import OracleCtx
    g, o = GpuCtx(), OracleCtx()
    rg = run_push(g, name, "gpu ")
    ro = run_push(o, name, "oracle ")
    g.close()
    o.close()
    assert rg == ro


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deterministic-lineitem",
                                  "random-lineitem"])
def test_q17_push_load_then_step_dev_gpu(name):
    """The benched path: `_push` as the load at t0, then `step_dev`
    churn over device-resident lineitem deltas (part idle), against the
    reference including the arr_avg / arr_dist peeks."""
    import torch
    from materialize_amd._ffi import GpuCtx
    steps, want = reference(name)
    g = GpuCtx()
    df = Q17Dataflow(g)
    push(df, 0, *steps[0])
    check_state(df, 0, want[0])
    dev = "cuda:0"
    for t, (lp, part) in enumerate(steps[1:], 1):
        assert not part
        k, v, d = lp_cols(lp)
        kt = torch.from_numpy(k).to(dev)
        vt = torch.from_numpy(np.ascontiguousarray(v).reshape(-1)).to(dev)
        tt = torch.full((len(k),), t, dtype=torch.int64, device=dev)
        dt = torch.from_numpy(d).to(dev)
        df.step_dev(abi.make_updates_from_torch(kt, vt, tt, dt, t, t + 1), t)
        check_state(df, t, want[t])
    g.close()
