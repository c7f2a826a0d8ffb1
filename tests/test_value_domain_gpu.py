"""The HIP engine over the whole value domain: full-width sort columns,
the sign boundary, partial val words with high bytes set, times >= 2^63,
the sort planner's 64-bit and 6-column chunk splits, the cached-plan
bounds where their padding saturates, and i128 sums at the i64 extremes.

Every result is held to two references: the naive tuple reference of
tests/valdomain.py (row for row, in order) and the CPU oracle (column for
column, byte for byte). tests/test_value_domain_cpu.py proves the same
inputs valid without a GPU and documents the generators; each case here
re-asserts the planner shape it exists for."""
import numpy as np
import pytest

import valdomain as vd
from materialize_amd import _abi as abi
from test_sort_plan_gpu import _dev_updates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    from materialize_amd._ffi import GpuCtx
    ctx = GpuCtx()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def o():
    from pyoracle import OracleCtx
    ctx = OracleCtx()
    yield ctx
    ctx.close()


def check_consolidate(g, o, kw, vb, batch, what):
    sch = abi.schema(kw, vb)
    got = g.consolidate(sch, vd.updates(abi, batch, 0, vd.U64_MAX))
    assert vd.to_rows(*got, kw, vb) == vd.naive_consolidated(batch, kw, vb), \
        f"{what}: GPU vs naive"
    want = o.consolidate(sch, vd.updates(abi, batch, 0, vd.U64_MAX))
    vd.assert_cols_equal(got, want, f"{what}: GPU vs oracle")


@pytest.mark.parametrize("name", sorted(vd.CONSOLIDATE_CASES))
def test_consolidate_case(g, o, name):
    kw, vb, batch = vd.make_case(name)
    vd.assert_case_shape(name, kw, vb, batch)
    check_consolidate(g, o, kw, vb, batch, name)


@pytest.mark.parametrize("kw,vb", vd.EDGE_GRID)
def test_consolidate_edge_values(g, o, kw, vb):
    batch = vd.gen_edges(np.random.default_rng(kw * 100 + vb), 1500, kw, vb)
    check_consolidate(g, o, kw, vb, batch, f"edges kw={kw} vb={vb}")


@pytest.mark.parametrize("name", sorted(vd.PLAN_SEQUENCES))
def test_cached_plan_sequence(g, o, name):
    """Device-staged inserts (the only path that caches the sort plan);
    after every flush the whole arrangement is read back."""
    seq = vd.make_sequence(name)
    trace = vd.plan_trace(seq)  # asserts covered / re-planned per batch
    if name == "pad_shift":
        assert trace[0] == ([[31, 33]], [[32], [33]])
    sch = abi.schema(1, 8)
    ga, oa = g.arr_create(sch), o.arr_create(sch)
    keep, batches = [], []
    for t, (b, _) in enumerate(seq):
        keys, vals, times, diffs = b
        du, refs = _dev_updates(keys, vals, times.view(np.int64), diffs,
                                t, t + 1)
        keep.append(refs)  # device inputs must outlive the flush
        g.arr_insert_async(ga, du)
        g.arr_flush(ga)
        o.arr_insert(oa, vd.updates(abi, b, t, t + 1))
        batches.append(b)
        got = g.peek_scan(ga, t, allow_negative=True)
        assert vd.to_rows(*got, 1, 8) == vd.naive_as_of(batches, t, 1, 8), \
            f"{name} t={t}: GPU vs naive"
        allkeys = np.unique(np.concatenate([x[0].ravel() for x in batches]))
        vd.assert_cols_equal(got, o.peek(oa, allkeys, t),
                             f"{name} t={t}: GPU scan vs oracle peek")


def check_reduce(got, want_oracle, want_model, kw, what):
    assert vd.to_rows(*got, kw, 48) == want_model, f"{what}: GPU vs model"
    vd.assert_cols_equal(got, want_oracle, f"{what}: GPU vs oracle")


def test_time_major_sort_full_width(g, o):
    """One multi-timestamp reduce push: the (time, key) sort runs three
    full-width chunks, and the per-time corrections must come out in
    time order."""
    batch = vd.gen_time_major(np.random.default_rng(7))
    assert vd.plan_shape(batch, 2, 0, time_major=True) == [vd.F] * 3
    spec = vd.sum_count_spec(abi, 2)
    gop, oop = g.reduce_create(spec), o.reduce_create(spec)
    u = vd.updates(abi, batch, 0, vd.U64_MAX)
    got = g.reduce_push(gop, u)
    check_reduce(got, o.reduce_push(oop, u),
                 vd.SumCountModel().push(batch, 2), 2, "time-major")
    g.reduce_drop(gop)


def test_sum_i64_at_the_extremes(g, o):
    """Plain SUM_I64 + COUNT: vals INT64_MIN / INT64_MAX under diffs +-1
    and +-2^62 over several pushes. The 16-byte slot is the Python
    integer sum mod 2^128, COUNT the diff sum mod 2^64 (SumCountModel)."""
    rng = np.random.default_rng(11)
    spec = vd.sum_count_spec(abi, 1)
    gop, oop = g.reduce_create(spec), o.reduce_create(spec)
    model = vd.SumCountModel()
    for t in range(5):
        batch = vd.gen_sum_extremes(rng, t)
        u = vd.updates(abi, batch, t, t + 1)
        check_reduce(g.reduce_push(gop, u), o.reduce_push(oop, u),
                     model.push(batch, 1), 1, f"push {t}")
    assert any(acc >= 2**127 for acc, _, _ in model.state.values())
    g.reduce_drop(gop)


@pytest.mark.parametrize("kw", [1, 2])
def test_probes_full_width_keys(g, o, kw):
    """halfjoin (le and lt) and keyed peek over an arrangement of
    full-width and sign-boundary keys."""
    rng = np.random.default_rng(20 + kw)
    batches = vd.gen_probe_arrangement(rng, kw)
    stream = vd.gen_probe_stream(rng, batches, kw)
    sch = abi.schema(kw, 8)
    ga, oa = g.arr_create(sch), o.arr_create(sch)
    for b in batches:
        u = vd.updates(abi, b, 0, vd.U64_MAX - 1)
        g.arr_insert(ga, u)
        o.arr_insert(oa, u)
    su = vd.updates(abi, stream, 3, vd.U64_MAX - 1)
    cl = vd.probe_closure(abi, kw)
    for le in (True, False):
        got = g.halfjoin(ga, su, 0, le, cl)
        assert vd.to_rows(*got, kw, 8) == \
            vd.naive_halfjoin(stream, batches, kw, le), f"le={le} vs naive"
        vd.assert_cols_equal(got, o.halfjoin(oa, su, 0, le, cl),
                             f"halfjoin le={le} vs oracle")
    pk = np.unique(stream[0], axis=0)
    asked = {tuple(k) for k in pk.tolist()}
    for as_of in (2, 2**63, vd.U64_MAX - 2):
        got = g.peek(ga, pk, as_of, kw)
        want = [r for r in vd.naive_as_of(batches, as_of, kw, 8)
                if r[0] in asked]
        assert vd.to_rows(*got, kw, 8) == want, f"peek {as_of} vs naive"
        vd.assert_cols_equal(got, o.peek(oa, pk, as_of, kw),
                             f"peek as_of={as_of} vs oracle")
