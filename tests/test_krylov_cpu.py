"""lanczos_tridiagonal, krylov_evolve_pauli_sum and lanczos_ground_state on the
CPU engine, through the wrapping layers and the generic lowering, plus the
host mathematics (krylov_coefficients) with no engine involved and the
example. Oracle and tolerances: krylov_oracle.py; the checks shared with the
HIP engine's file are in krylov_cases.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import krylov_oracle as ko
import krylov_cases as kc

ENGINE = "cpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = kc.PRECS


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    kc.widths(ENGINE, n, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("x", kc.ac.x_masks_12(), ids=lambda x: "x%03x" % x)
def test_partner_logic_12(x, prec):
    kc.partner_logic(ENGINE, prec, x)


@pytest.mark.parametrize("prec", PRECS)
def test_group_larger_than_cap_splits(prec):
    kc.chunking(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dim", kc.DIMS)
def test_dims(dim, prec):
    kc.dims(ENGINE, prec, dim)


@pytest.mark.parametrize("prec", PRECS)
def test_error_estimate(prec):
    kc.estimate_cases(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_breakdown(prec):
    kc.breakdown(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_stepping_and_edge_inputs(prec):
    kc.stepping_and_edges(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_read_only_and_repeatable(prec):
    kc.readonly_and_repeatable(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_argument_errors(prec):
    kc.argument_errors(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_ground_state_restarts(prec):
    kc.ground_state(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "cpu"]), ids=lambda l: "-".join(l))
def test_layers_reach_engine(layers, prec):
    kc.layers_match_engine(ENGINE, layers, prec, 9, 64 * kc.EPS[prec])


# lossless stacks over the host-copy lowering reproduce the engine to rounding;
# turboquant stores 16-bit codes, so the state it hands back after a mutating
# call is rounded to its own grid
LOWERED = (
    (["qunit", "cpu"], 1e-5),
    (["pager", "cpu"], 1e-5),
    (["stabilizer_hybrid", "cpu"], 1e-5),
    (["bdt"], 1e-5),
    (["sparse"], 1e-5),
    (["tensor_network", "cpu"], 1e-5),
    (["turboquant"], 2e-3),
)


@pytest.mark.parametrize("layers,tol", LOWERED, ids=["-".join(l) for l, _ in LOWERED])
def test_lowering_matches_engine(layers, tol):
    kc.layers_match_engine(ENGINE, layers, "fp32", 6, tol)


def test_noise_layer(monkeypatch):
    monkeypatch.setenv("QRACK_GATE_DEPOLARIZATION", "0.0")
    n = 4
    terms = kc.chain_terms(n)
    q = qa.create_simulator(n, layers=["noisy", "cpu"], seed=3)
    psi = kc.random_psi(n, "fp32", seed=811)
    q.set_state_vector(psi)
    with pytest.raises(Exception, match="not defined under gate noise"):
        q.krylov_evolve_pauli_sum(terms, 0.1, 4)
    with pytest.raises(Exception, match="not defined under gate noise"):
        q.lanczos_ground_state(terms, 4, True)
    assert kc.state_of(q).tobytes() == psi.tobytes()
    # the read-only forms are forwarded
    kc.check_tridiagonal(q, psi, terms, 4, "fp32", "noisy")
    bare = kc.sim(ENGINE, n, "fp32")
    bare.set_state_vector(psi)
    assert q.lanczos_ground_state(terms, 4, False) == bare.lanczos_ground_state(terms, 4, False)


# ---- host mathematics ----------------------------------------------------------------


@pytest.mark.parametrize("k", (1, 2, 7, 64))
def test_krylov_coefficients_against_eigh(k):
    rng = np.random.default_rng(40 + k)
    alpha = rng.uniform(-2, 2, k)
    beta = rng.uniform(0.1, 2, k)  # the last entry is beta_(k+1): ignored
    for time in (0.7, -1.3):
        got = qa.krylov_coefficients(alpha, beta, time)
        want = ko.coefficients(alpha, beta, time)
        err = float(np.abs(got - want).max())
        print(f"k = {k}, time = {time}: max err = {err:.3e}, | |c| - 1 | = {abs(np.linalg.norm(got) - 1):.3e}")
        assert got.shape == (k,) and err <= 1e-12
        assert abs(np.linalg.norm(got) - 1.0) <= 1e-12
        # beta without the trailing entry is accepted too
        assert np.array_equal(qa.krylov_coefficients(alpha, beta[:k - 1], time), got)
    assert np.abs(qa.krylov_coefficients(alpha, beta, 0.0) - np.eye(k)[0]).max() <= 1e-15
    with pytest.raises(Exception):
        qa.krylov_coefficients([], [], 0.1)
    with pytest.raises(Exception):
        qa.krylov_coefficients(alpha, beta[:max(k - 2, 0)], 0.1) if k > 1 else qa.krylov_coefficients([], [], 0.1)
    assert qa.KRYLOV_COMBINE_MAX_VECTORS >= 1


# ---- example --------------------------------------------------------------------------


def test_krylov_quench_example():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "krylov_quench.py")],
                       capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")})
    assert r.returncode == 0, f"stdout={r.stdout}\nstderr={r.stderr}"
    assert "krylov" in r.stdout.lower()
