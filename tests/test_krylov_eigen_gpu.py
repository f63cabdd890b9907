"""lanczos_lowest_states on the HIP engine: k_krylov_orth over 1 to 64 vectors
(the inner-product pass, the update fused with the next inner products or the
norm, one and several chunks) and the in-place k_krylov_rotate at every basis
and output count of eigen_cases.TRACKING.

Oracle and tolerances: eigen_oracle.py (numpy on the engine's own
get_state_vector()); the checks shared with the CPU engine's file are in
eigen_cases.py. The child processes pin what only a fresh process can: the
launch counts under QRACK_PROFILE, the stride loops under QRACK_GPU_BLOCKS and
the memory peaks under QRACK_MAX_ALLOC_MB.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import adjoint_oracle as ao
import krylov_cases as kc
import eigen_cases as ec

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ENGINE = "hip"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ec.PRECS


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


@pytest.mark.parametrize("prec", PRECS)
def test_prepared_vectors(prec):
    ec.prepared_vectors(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_read_only_and_repeatable(prec):
    ec.readonly_and_repeatable(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    """One item or two (1, 2), fewer items than a wave (5), several blocks (9)."""
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


# ---- child processes ------------------------------------------------------------------


def run_child(fn, env, *args):
    code = ("import os, sys\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
            "import test_krylov_eigen_gpu as t\n"
            f"t.{fn}(*sys.argv[2:])\n")
    r = subprocess.run(
        [sys.executable, "-c", code, ROOT, *args],
        env={**os.environ, **env}, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, f"stdout={r.stdout}\nstderr={r.stderr}"
    return r.stdout


# launch counts, on the bare engine and through the layers

PROFILE_N = 9
# (name, nev, dim, max_restarts, prepare)
PROFILE_CALLS = (("plain", 3, 12, 2, -1), ("prepare", 3, 12, 2, 1), ("no_restart", 2, 8, 0, 0),
                 ("chunks", 8, 34, 1, -1), ("chunks_prepare", 8, 34, 1, 7))


def krylov_counts():
    return {key: int(v[0]) for key, v in qa.profile_report().items() if key.startswith("krylov")}


def child_profile():
    """run under QRACK_PROFILE=1: launch counts of one call each, as JSON"""
    terms = kc.chain_terms(PROFILE_N)
    psi = kc.random_psi(PROFILE_N, "fp32")
    report = {}
    for name, nev, dim, rs, prepare in PROFILE_CALLS:
        q = kc.sim(ENGINE, PROFILE_N, "fp32")
        q.set_state_vector(psi)
        qa.profile_reset()
        _, _, info = ec.call(q, terms, nev, dim, 0.0, rs, prepare)
        report[name] = {"restarts": int(info["restarts"]), "applies": int(info["applies"]),
                        "counts": krylov_counts()}
    layers = {}
    for stack in (["hybrid"], ["fuser", "hip"]):
        bare = kc.sim(ENGINE, PROFILE_N, "fp32")
        q = kc.sim(ENGINE, PROFILE_N, "fp32", layers=stack)
        q.set_state_vector(psi)
        bare.set_state_vector(kc.state_of(q))
        qa.profile_reset()
        v, r, info = ec.call(q, terms, 2, 6, 0.0, 3)
        counts = krylov_counts()
        wv, wr, winfo = ec.call(bare, terms, 2, 6, 0.0, 3)
        layers["-".join(stack)] = {"counts": counts, "restarts": int(info["restarts"]),
                                   "dev": float(max(np.abs(v - wv).max(), np.abs(r - wr).max()))}
    print("REPORT " + json.dumps(report))
    print("LAYERS " + json.dumps(layers))


@pytest.fixture(scope="module")
def profile_report():
    # the hybrid layer hands a 9-qubit state to the HIP engine only when told to
    out = run_child("child_profile", {"QRACK_PROFILE": "1", "QRACK_GPU_THRESHOLD_QB": "1"})
    rep = json.loads([l for l in out.splitlines() if l.startswith("REPORT ")][-1][len("REPORT "):])
    lay = json.loads([l for l in out.splitlines() if l.startswith("LAYERS ")][-1][len("LAYERS "):])
    return rep, lay


def test_profile_counts_the_launches(profile_report):
    """applies * L of krylov_apply, the orth launches of the chunk rule, one
    krylov_rotate per restart, krylov_combine only with prepare >= 0"""
    launches = ao.launches(kc.chain_terms(PROFILE_N))
    assert launches >= 3
    for name, nev, dim, rs, prepare in PROFILE_CALLS:
        got = profile_report[0][name]
        assert got["restarts"] == rs, name
        steps = ec.steps_of(nev, dim, rs)
        assert got["applies"] == len(steps)
        # after a restart the basis holds no state: all dim vectors are sources
        want = ec.expected_launches(steps, launches, rs, dim if prepare >= 0 else None, state_in_basis=rs == 0)
        assert got["counts"] == want, (name, got["counts"], want)
    assert ec.expected_launches(ec.steps_of(8, 34, 1), launches, 1, 34, False)["krylov_combine"] == 3


def test_layers_reach_engine(profile_report):
    """["hybrid"] and ["fuser", "hip"] return the bare engine's values (the
    fp32 state tolerance of the GPU suite) and run the engine's own kernels"""
    s = ec.ko.sum_abs(kc.chain_terms(PROFILE_N))
    for stack, got in profile_report[1].items():
        assert got["dev"] <= 2e-4 * s, (stack, got)
        assert got["counts"].get("krylov_orth", 0) == sum(
            ec.eo.orth_launches(j) for j in ec.steps_of(2, 6, got["restarts"])), (stack, got)


@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "hip"]), ids=lambda l: "-".join(l))
def test_layers_match_engine(layers):
    ec.layers_match_engine(ENGINE, layers, "fp32", 9, 2e-4)


# stride loops


def child_stride():
    """run under QRACK_GPU_BLOCKS=2: 512 threads for 256 (fp32) or 512 (fp64)
    items of 16 bytes would be one trip, so 11 qubits: a second trip of every
    stride loop; and the 9-qubit tracking cases, where the cap halves the grid"""
    for prec in PRECS:
        for case in ((3, 12, 3), (4, 17, 2), (8, 34, 1)):
            ec.tracking(ENGINE, prec, case)
        stride_11(prec)
    print("CHILD_OK")


def stride_11(prec):
    n = 11
    terms = kc.chain_terms(n)
    psi = kc.random_psi(n, prec, seed=1100)
    want = ec.eo.lowest_states(psi, terms, 4, 17, 0.0, 1, prec)
    q = kc.sim(ENGINE, n, prec)
    q.set_state_vector(psi)
    v, r, info = ec.call(q, terms, 4, 17, 0.0, 1)
    # the tracking tolerance, for this case
    p32 = psi.astype(np.complex64)
    a = ec.eo.lowest_states(p32, terms, 4, 17, 0.0, 1, "fp32", np.complex64)
    b = ec.eo.lowest_states(p32, terms, 4, 17, 0.0, 1, "fp32")
    d = max(np.abs(a["values"] - b["values"]).max(), np.abs(a["residuals"] - b["residuals"]).max())
    tol = max(8 * d * ec.ko.scale_to(prec), 16 * ec.EPS[prec] * ec.ko.sum_abs(terms))
    err = max(np.abs(v - want["values"]).max(), np.abs(r - want["residuals"]).max())
    print(f"stride 11/{prec}: err = {err:.3e}, tol = {tol:.3e}")
    assert info["restarts"] == 1 and err <= tol


def test_stride_loops_in_child():
    assert "CHILD_OK" in run_child("child_stride", {"QRACK_GPU_BLOCKS": "2"})


# memory peaks

ALLOC_N = 20  # 8 MiB per fp32 state
ALLOC_DIM = 4


def child_alloc(expect, max_restarts):
    """run under QRACK_MAX_ALLOC_MB at 20 qubits fp32: `expect` says whether
    the cap admits the call's buffers"""
    q = kc.sim(ENGINE, ALLOC_N, "fp32")
    for b in range(ALLOC_N):
        q.ry(0.3 + 0.05 * b, b)
        q.rz(0.2 + 0.03 * b, b)
    terms = kc.chain_terms(ALLOC_N)
    before = kc.state_of(q)
    try:
        v, r, info = ec.call(q, terms, 1, ALLOC_DIM, 0.0, int(max_restarts))
        fitted = True
    except Exception:
        fitted = False
    assert fitted == (expect == "fits")
    assert kc.state_of(q).tobytes() == before.tobytes()
    if fitted:
        assert len(v) == 1 and np.isfinite(v[0]) and info["applies"] == ALLOC_DIM + 2 * int(max_restarts)
        print("FITS")
    else:
        print("REFUSED_STATE_INTACT")


def test_peaks_at_dim_plus_one_states_without_restarts():
    """40 MiB hold the state and the dim = 4 buffers; 39 MiB are one state short"""
    assert "FITS" in run_child("child_alloc", {"QRACK_MAX_ALLOC_MB": "40"}, "fits", "0")
    assert "REFUSED_STATE_INTACT" in run_child("child_alloc", {"QRACK_MAX_ALLOC_MB": "39"}, "refused", "0")


def test_restarts_take_one_more_state():
    """after a restart all dim vectors and w are the call's own: dim + 2 states"""
    assert "FITS" in run_child("child_alloc", {"QRACK_MAX_ALLOC_MB": "48"}, "fits", "2")
    assert "REFUSED_STATE_INTACT" in run_child("child_alloc", {"QRACK_MAX_ALLOC_MB": "47"}, "refused", "2")
