"""The QFT oracle held to itself, then the CPU engine (and the pager over
it) held to the oracle: qft / iqft over the whole case table of
qft_cases.py, and the ramp primitives the pagers build their transforms
from. Tolerance and its derivation: qft_cases.py.
"""

import numpy as np
import pytest

import qrack_amd as qa
import gate_oracle as go
import qft_cases as qc
import qft_oracle as qo


def _need_long(precision):
    if precision == "fp64" and not qo.LONG_OK:
        pytest.skip(qc.LONG_SKIP)


# ---- the oracle against itself ------------------------------------------------------

@pytest.mark.parametrize("n", (3, 8, 12))
def test_oracle_is_the_bit_reversed_dft(n):
    v = go.random_state(n, np.random.default_rng(n))
    got = qo.qft(qo.work(v), 0, n)
    # the closed form is a complex128 FFT: it is the looser side here
    assert np.abs(got - qo.dft_bitrev(v, n)).max() < 1e-15
    assert np.abs(qo.qft(qo.work(v, long=False), 0, n) - qo.dft_bitrev(v, n)).max() < 1e-15


def test_oracle_is_the_gate_product():
    """Bits 1..4 of 5 qubits: H and controlled phases one at a time,
    through gate_oracle.State, in the order of QInterface::QFT."""
    n, start, length = 5, 1, 4
    v = go.random_state(n, np.random.default_rng(17))
    st = go.State(v)
    for i in range(length - 1, -1, -1):
        st.mtrx(np.array([1, 1, 1, -1]) / np.sqrt(2), start + i)
        for j in range(i):
            st.mcphase([start + j], 1, np.exp(1j * np.pi / (1 << (i - j))), start + i)
    assert np.abs(qo.qft(qo.work(v), start, length) - st.v).max() < 1e-15
    assert np.abs(qo.qftr(qo.work(v), list(range(start, start + length))) - st.v).max() < 1e-15


@pytest.mark.parametrize("start,length,n", ((0, 12, 12), (3, 6, 10), (13, 1, 14)))
def test_oracle_inverse_undoes_forward(start, length, n):
    v = qo.work(go.random_state(n, np.random.default_rng(3)))
    back = qo.qft(qo.qft(v.copy(), start, length), start, length, inverse=True)
    assert np.abs(back - v).max() < 64 * qo.LONG_EPS


def test_dropping_a_term_moves_the_state():
    """The figure the tolerance condition rests on: without the pi / 2^11
    phase of the top column a 12-qubit transform moves by about 7.5e-4."""
    case = qc.CASES["fp32"][[c.id for c in qc.CASES["fp32"]].index("n12")]
    d = qc.drop_distance(case, "qft", "fp32")
    assert 5e-4 < d < 1e-3
    assert d > 400 * 12 * qc.EPS["fp32"]


def test_primitives_are_their_gate_products():
    """phase_ramp_general and qft_column_general against per-bit phases."""
    n = 10
    v = go.random_state(n, np.random.default_rng(23))
    scale, mask, pows, ws, cond = np.pi / 128, 0b1011, [1 << 6, 1 << 8], [16, 64], 1 << 4
    st = go.State(v)
    for bit, w in ((0, 1), (1, 2), (3, 8), (6, 16), (8, 64)):
        st.mcphase([4], 1, np.exp(1j * scale * w), bit)
    got = qo.phase_ramp_general(qo.work(v), scale, 0, mask, pows, ws, cond)
    assert np.abs(got - st.v).max() < 1e-15
    st = go.State(v)
    st.mtrx(np.array([1, 1, 1, -1]) / np.sqrt(2), 4)
    for bit, w in ((0, 1), (1, 2), (3, 8), (6, 16), (8, 64)):
        st.mcphase([4], 1, np.exp(1j * scale * w), bit)
    st.phase(1, np.exp(0.3j), 4)
    got = qo.qft_column_general(qo.work(v), 4, scale, 0, mask, pows, ws, 0.3, False)
    assert np.abs(got - st.v).max() < 1e-15
    got = qo.phase_ramp(qo.work(v), scale, 3, 5, 0)
    ref = qo.phase_ramp_general(qo.work(v), scale, 3, 0b11111, [], [], 0)
    assert np.array_equal(got, ref)


# ---- declared plans against the planner ------------------------------------------------

def _plan(case, precision, **kw):
    return [tuple(p) for p in qa.qft_pass_plan(case.length, case.n, precision,
                                               start=case.start, **kw)]


@pytest.mark.parametrize("precision", qc.PRECISIONS)
def test_declared_plans_are_the_planners(precision):
    for case in qc.TABLE[precision]:
        if case.plan is not None:
            assert _plan(case, precision) == qc.parse_plan(case.plan), case.id
    for name, (_env, kw, per) in qc.SWITCHES.items():
        for case in per[precision]:
            assert _plan(case, precision, **kw) == qc.parse_plan(case.plan), (name, case.id)


def test_plan_keywords_default_to_the_engines_defaults():
    for n in (6, 13, 17, 21):
        for precision in qc.PRECISIONS:
            assert (qa.qft_pass_plan(n, n, precision)
                    == qa.qft_pass_plan(n, n, precision, 9, start=0, fuse=4, lds_low=True,
                                        lds_mid=True))
    with pytest.raises(ValueError):
        qa.qft_pass_plan(5, 8, "fp32", start=4)


# ---- the CPU engine ----------------------------------------------------------------------

_sims = {}


def make(n, precision, layers=()):
    key = (n, precision, tuple(layers))
    if key not in _sims:
        if layers:
            _sims[key] = qa.create_simulator(n, precision=precision, seed=7,
                                             layers=list(layers) + ["cpu"],
                                             pages_per_device=qc.PAGES_PER_DEVICE)
        else:
            _sims[key] = qa.create_simulator(n, precision=precision, engine="cpu", seed=7)
    return _sims[key]


def _params(table):
    return [pytest.param(p, c, op, id=f"{c.id}-{op}-{p}")
            for p in qc.PRECISIONS for c in table(p) for op in c.ops]


@pytest.mark.parametrize("precision,case,op", _params(lambda p: qc.TABLE[p] + qc.PAGER_CASES))
def test_cpu_engine_vs_oracle(precision, case, op):
    _need_long(precision)
    q = make(case.n, precision, case.layers or ())
    got = qc.run(q, case, op, precision)
    qc.check(got, qc.expected(case, op, precision), precision, case.length,
             label=f"{case.id} {op}")
    if qc.full_ladder(case, precision):
        qc.check_floor(case, op, precision, qc.C_DERIVED)


@pytest.mark.parametrize("precision", qc.PRECISIONS)
@pytest.mark.parametrize("prim_id", [p.id for p in qc.PRIMS if not p.hip_only])
def test_cpu_primitive_vs_oracle(prim_id, precision):
    _need_long(precision)
    prim = qc.PRIM_BY_ID[prim_id]
    got = qc.run_prim(make(prim.n, precision), prim, precision)
    qc.check(got, qc.prim_expected(prim_id, precision), precision, prim.cols, label=prim_id)
