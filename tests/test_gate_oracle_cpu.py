"""Gate path of the CPU engine against the numpy oracle in gate_oracle.py.
Case table, tolerance and checks: gate_cases.py, shared with
test_gate_oracle_gpu.py.

This keeps the oracle and the conventions it encodes (bit order, 4x4 basis
order, fsim and cphase signs, multiplexer selection order, list-order
fallbacks) checked on machines with no GPU: every case of the table,
the capped-grid cases and the single-target cases of the HIP switches run
here as plain cases. On this engine the largest error over the table is
1.48 G eps a in fp32 and 1.65 G eps a in fp64 (4x4 gates), against the
derived bound of 3.
"""

import numpy as np
import pytest

import qrack_amd as qa
import gate_cases as gc
import gate_oracle as go


def make(n, precision):
    return qa.create_simulator(n, precision=precision, engine="cpu", seed=7)


@pytest.mark.parametrize("precision", gc.PRECISIONS)
@pytest.mark.parametrize("case_id", gc.IDS)
def test_gate_vs_oracle(case_id, precision):
    case = gc.BY_ID[precision][case_id]
    gc.run_case(make(case.n, precision), case, precision)


@pytest.mark.parametrize("precision", gc.PRECISIONS)
def test_wide_and_switch_cases(precision):
    """The 14-qubit capped-grid cases and the cases of the WIDE / NT / MFMA
    children, on this engine."""
    cases = list(gc.STRIDE_CASES[precision])
    if precision == "fp32":
        cases += gc.WIDE_CASES + gc.NT_CASES + gc.MFMA_CASES
    for case in cases:
        gc.run_case(make(case.n, precision), case, precision)


@pytest.mark.parametrize("precision", gc.PRECISIONS)
def test_state_round_trip_is_bit_exact(precision):
    state = go.random_state(10, np.random.default_rng(5)).astype(gc.DTYPE[precision])
    q = make(10, precision)
    q.set_state_vector(state)
    assert np.array_equal(np.asarray(q.get_state_vector()), state)


def test_table_reaches_every_route():
    """Every host route name is declared by at least one batch case in each
    precision, so the profile child has something to hold each kernel to."""
    for precision in gc.PRECISIONS:
        seen = set()
        for case in gc.CASES[precision]:
            seen |= set(case.routes or ())
        assert seen == set(gc.ROUTE_OPS), set(gc.ROUTE_OPS) - seen


def test_oracle_self_consistency():
    """The oracle against itself: a 4x4 built from two 2x2s equals the two
    2x2s, on either qubit order, and a controlled gate leaves the rest alone."""
    rng = np.random.default_rng(11)
    v = go.random_state(6, rng)
    u1, u2 = gc._unitary(rng, 2), gc._unitary(rng, 2)
    a = go.State(v)
    a.mtrx(u1, 4)
    a.mtrx(u2, 1)
    for q1, q2, m in ((4, 1, np.kron(u2, u1)), (1, 4, np.kron(u1, u2))):
        b = go.State(v)
        b.mtrx_2q(m, q1, q2)
        assert np.allclose(a.v, b.v, rtol=0, atol=1e-15)
    c = go.State(v)
    c.mcmtrx([0, 5], u1, 3)
    idx = np.arange(64)
    off = (idx & 0b100001) != 0b100001
    assert np.array_equal(c.v[off], v[off]) and not np.any(c.v[~off] == v[~off])
