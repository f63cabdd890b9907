"""lanczos_lowest_states on the CPU engine, through the wrapping layers and the
generic lowering, plus the example. Oracle and tolerances: eigen_oracle.py;
the checks shared with the HIP engine's file are in eigen_cases.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import krylov_cases as kc
import krylov_oracle as ko
import eigen_cases as ec
import eigen_oracle as eo

ENGINE = "cpu"
PRECS = ec.PRECS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", ec.TRACKING, ids=lambda c: "nev%d-dim%d-r%d" % c)
def test_tracks_the_oracle(case, prec):
    ec.tracking(ENGINE, prec, case)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nev,dim", ec.DENSE)
def test_dense_spectrum_with_tolerance(nev, dim, prec):
    ec.dense_spectrum(ENGINE, prec, nev, dim)


@pytest.mark.parametrize("prec", PRECS)
def test_dense_spectrum_to_rounding(prec):
    ec.dense_spectrum(ENGINE, prec, 3, 12, tol=0.0, max_restarts=64)


def test_four_distinct_levels_at_dim_64_in_fp32():
    ec.flagship(ENGINE)


def test_plain_lanczos_shows_ghosts_there():
    """what the flagship case is about, on the oracle alone: plain Lanczos at
    dim 64 in complex64 returns the ground level twice"""
    terms, s, lam = ec.chain()
    a, b, _, _ = ko.lanczos(kc.random_psi(ec.N, "fp32"), terms, 64, "fp32", np.complex64)
    ritz = np.linalg.eigvalsh(ko.tridiag(a, b))[:4]
    assert abs(ritz[1] - lam[0]) <= 64 * ko.EPS["fp32"] * s < abs(ritz[1] - lam[1])


@pytest.mark.parametrize("prec", PRECS)
def test_prepared_vectors(prec):
    ec.prepared_vectors(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_read_only_and_repeatable(prec):
    ec.readonly_and_repeatable(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    ec.widths(ENGINE, n, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_breakdown(prec):
    ec.breakdown(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_any_norm(prec):
    ec.any_norm(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_argument_errors(prec):
    ec.argument_errors(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "cpu"]), ids=lambda l: "-".join(l))
def test_layers_reach_engine(layers, prec):
    ec.layers_match_engine(ENGINE, layers, prec, 9, 64 * ec.EPS[prec])


def test_qunit_stack_matches_through_the_lowering():
    ec.layers_match_engine(ENGINE, ["qunit", "cpu"], "fp32", 6, 1e-5)


def test_noise_layer(monkeypatch):
    monkeypatch.setenv("QRACK_GATE_DEPOLARIZATION", "0.0")
    n = 4
    terms = kc.chain_terms(n)
    q = qa.create_simulator(n, layers=["noisy", "cpu"], seed=3)
    psi = kc.random_psi(n, "fp32", seed=811)
    q.set_state_vector(psi)
    with pytest.raises(Exception, match="not defined under gate noise"):
        q.lanczos_lowest_states(terms, 2, 6, 0.0, 4, 0)
    v, r, info = ec.call(q, terms, 2, 6, 0.0, 4)
    bare = kc.sim(ENGINE, n, "fp32")
    bare.set_state_vector(kc.state_of(q))
    assert ec.blob(v, r, info) == ec.blob(*ec.call(bare, terms, 2, 6, 0.0, 4))


def test_keep_and_launch_rules():
    assert [eo.keep_rule(*c[:2]) for c in ec.TRACKING] == [6, 4, 1, 8, 8, 8, 16, 16, 16, 16, 16, 13]
    assert [eo.orth_launches(j) for j in (1, 16, 17, 32, 33, 48, 49, 64)] == [3, 3, 8, 8, 12, 12, 16, 16]
    assert ec.steps_of(3, 12, 1) == list(range(1, 13)) + list(range(7, 13))


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "spectral_gap.py"), "--qubits", "6",
                        "--engine", "cpu", "--points", "3"],
                       capture_output=True, text=True, timeout=120,
                       env={**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")})
    assert r.returncode == 0, r.stderr
    assert "gap" in r.stdout
