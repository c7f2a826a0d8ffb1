"""CPU companion of test_value_domain_gpu.py: every generator of
tests/valdomain.py runs through the oracle against the naive tuple
reference, so the inputs the GPU tests use are proven valid (and the
oracle proven right on them) without a GPU. The planner-shape model is
asserted here too: each case must produce the chunk layout it exists
for."""
import numpy as np
import pytest

import valdomain as vd
from materialize_amd import _abi as abi
from pyoracle import OracleCtx


@pytest.fixture(scope="module")
def o():
    ctx = OracleCtx()
    yield ctx
    ctx.close()


def test_planner_model_chunking():
    """The model itself, on hand-built spans: 64-bit limit, exact fit,
    6-column limit, constant columns dropped, saturating padding."""
    assert vd.chunk_bits([(0, 2**64 - 1)]) == [[64]]
    assert vd.chunk_bits([(5, 5), (1, 2**32 + 1), (0, 2**31)]) == \
        [[33], [32]]
    assert vd.chunk_bits([(0, 2**32 - 1)] * 2) == [[32, 32]]
    assert vd.chunk_bits([(0, 3)] * 13) == [[2] * 6, [2] * 6, [2]]
    assert vd.chunk_bits([(9, 9)] * 4) == []
    assert vd.pad_spans([(10, 1000), (7, 7), (2**64 - 120, 2**64 - 10)]) == \
        [(0, 1124), (7, 7), (2**64 - 134, 2**64 - 1)]
    assert vd.covered([(0, 10), (3, 3)], [(2, 9), (8, 8)])
    assert not vd.covered([(0, 10), (3, 3)], [(2, 9), (8, 9)])
    assert not vd.covered([(0, 10), (3, 3)], [(2, 11), (3, 3)])


@pytest.mark.parametrize("name", sorted(vd.CONSOLIDATE_CASES))
def test_consolidate_case_oracle_matches_naive(o, name):
    kw, vb, batch = vd.make_case(name)
    vd.assert_case_shape(name, kw, vb, batch)
    got = o.consolidate(abi.schema(kw, vb),
                        vd.updates(abi, batch, 0, vd.U64_MAX))
    want = vd.naive_consolidated(batch, kw, vb)
    assert vd.to_rows(*got, kw, vb) == want
    # every column that varies decides the order of some pair of rows
    varying, deciding = vd.deciding_columns(want)
    assert deciding == varying, name


def test_consolidate_cases_cancel_and_split_on_msb():
    """The generators really plant cancelling duplicates and rows that
    differ in the most significant column only."""
    kw, vb, batch = vd.make_case("full_kw2_vb16")
    rows = vd.to_rows(*batch, kw, vb)
    out = vd.naive_consolidated(batch, kw, vb)
    assert len(out) < len({r[:3] for r in rows})  # some rows cancel to 0
    tails = {}
    for k, v, t, _ in out:
        tails.setdefault((k[1:], v, t), set()).add(k[0])
    assert sum(len(s) > 1 for s in tails.values()) > 20


@pytest.mark.parametrize("kw,vb", vd.EDGE_GRID)
def test_edge_values_oracle_matches_naive(o, kw, vb):
    batch = vd.gen_edges(np.random.default_rng(kw * 100 + vb), 1500, kw, vb)
    got = o.consolidate(abi.schema(kw, vb),
                        vd.updates(abi, batch, 0, vd.U64_MAX))
    assert vd.to_rows(*got, kw, vb) == vd.naive_consolidated(batch, kw, vb)


@pytest.mark.parametrize("name", sorted(vd.PLAN_SEQUENCES))
def test_plan_sequence_oracle_matches_naive(o, name):
    seq = vd.make_sequence(name)
    trace = vd.plan_trace(seq)
    if name == "pad_shift":  # exact spans: one 64-bit chunk; padded: two
        assert trace[0] == ([[31, 33]], [[32], [33]])
        assert trace[1][1] == [[32], [33]]
    if name in ("high", "low"):  # the padding saturated
        cached = vd.pad_spans(vd.column_spans(seq[0][0], 1, 8))
        assert cached[2][1 if name == "high" else 0] == \
            (vd.U64_MAX if name == "high" else 0)
    arr = o.arr_create(abi.schema(1, 8))
    batches = [b for b, _ in seq]
    for t, b in enumerate(batches):
        assert len(b[2]) <= 2000
        o.arr_insert(arr, vd.updates(abi, b, t, t + 1))
    last = len(batches) - 1
    allkeys = np.unique(np.concatenate([b[0].ravel() for b in batches]))
    assert vd.to_rows(*o.peek(arr, allkeys, last), 1, 8) == \
        vd.naive_as_of(batches, last, 1, 8)


def test_time_major_reduce_oracle_matches_model(o):
    batch = vd.gen_time_major(np.random.default_rng(7))
    assert vd.plan_shape(batch, 2, 0, time_major=True) == [vd.F] * 3
    op = o.reduce_create(vd.sum_count_spec(abi, 2))
    got = o.reduce_push(op, vd.updates(abi, batch, 0, vd.U64_MAX))
    want = vd.SumCountModel().push(batch, 2)
    assert len(want) > 500
    assert vd.to_rows(*got, 2, 48) == want


def test_sum_extremes_oracle_matches_model(o):
    rng = np.random.default_rng(11)
    op = o.reduce_create(vd.sum_count_spec(abi, 1))
    model = vd.SumCountModel()
    for t in range(5):
        batch = vd.gen_sum_extremes(rng, t)
        got = o.reduce_push(op, vd.updates(abi, batch, t, t + 1))
        assert vd.to_rows(*got, 1, 48) == model.push(batch, 1), f"push {t}"
    # the sums really left the i64 and the i128 range on the way
    assert any(acc >= 2**127 for acc, _, _ in model.state.values())


@pytest.mark.parametrize("kw", [1, 2])
def test_probe_inputs_oracle_matches_naive(o, kw):
    rng = np.random.default_rng(20 + kw)
    batches = vd.gen_probe_arrangement(rng, kw)
    stream = vd.gen_probe_stream(rng, batches, kw)
    arr = o.arr_create(abi.schema(kw, 8))
    for b in batches:
        o.arr_insert(arr, vd.updates(abi, b, 0, vd.U64_MAX - 1))
    su = vd.updates(abi, stream, 3, vd.U64_MAX - 1)
    cl = vd.probe_closure(abi, kw)
    res = {le: vd.to_rows(*o.halfjoin(arr, su, 0, le, cl), kw, 8)
           for le in (True, False)}
    for le in (True, False):
        assert res[le] == vd.naive_halfjoin(stream, batches, kw, le), le
    assert res[True] != res[False]
    pk = np.unique(stream[0], axis=0)
    asked = {tuple(k) for k in pk.tolist()}
    for as_of in (2, 2**63, vd.U64_MAX - 2):
        want = [r for r in vd.naive_as_of(batches, as_of, kw, 8)
                if r[0] in asked]
        assert vd.to_rows(*o.peek(arr, pk, as_of, kw), kw, 8) == want, as_of
