"""lanczos_tridiagonal, krylov_evolve_pauli_sum and lanczos_ground_state on the
HIP engine: the fused Lanczos step (k_krylov_apply in its three pair modes and
its diagonal form, FIRST and accumulating; k_krylov_finish with and without
its store) and k_krylov_combine across its launch boundaries.

Oracle and tolerances: krylov_oracle.py (numpy on the engine's own
get_state_vector()); the checks shared with the CPU engine's file are in
krylov_cases.py. The child processes pin what only a fresh process can: the
launch counts under QRACK_PROFILE, the stride loops under QRACK_GPU_BLOCKS and
the dim + 1 / 4 state peaks under QRACK_MAX_ALLOC_MB.
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

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ENGINE = "hip"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = kc.PRECS
N12 = kc.N12


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    """One vector or fewer (1, 2), fewer items than a wave (5), several blocks (9)."""
    kc.widths(ENGINE, n, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("x", kc.ac.x_masks_12(), ids=lambda x: "x%03x" % x)
def test_partner_logic_12(x, prec):
    """Every pair mode, alone (FIRST) and behind another group (accumulating)."""
    kc.partner_logic(ENGINE, prec, x)


@pytest.mark.parametrize("prec", PRECS)
def test_group_larger_than_cap_splits(prec):
    kc.chunking(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dim", kc.DIMS)
def test_dims(dim, prec):
    """1, 2, each side of every combine-launch boundary, and the largest."""
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


@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "hip"]), ids=lambda l: "-".join(l))
def test_layers_reach_engine(layers):
    # fp32 state tolerance of the GPU suite
    kc.layers_match_engine(ENGINE, layers, "fp32", 9, 2e-4)


# ---- child processes ------------------------------------------------------------------


def run_child(fn, env, *args):
    code = ("import os, sys\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
            "import test_krylov_gpu as t\n"
            f"t.{fn}(*sys.argv[2:])\n")
    r = subprocess.run(
        [sys.executable, "-c", code, ROOT, *args],
        env={**os.environ, **env}, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, f"stdout={r.stdout}\nstderr={r.stderr}"
    return r.stdout


# launch counts

PROFILE_N = 9


def child_profile():
    """run under QRACK_PROFILE=1: launch counts of one call each, as JSON"""
    terms = kc.chain_terms(PROFILE_N)
    psi = kc.random_psi(PROFILE_N, "fp32")
    report = {}

    def counted(name, call):
        q = kc.sim(ENGINE, PROFILE_N, "fp32")
        q.set_state_vector(psi)
        k = len(q.lanczos_tridiagonal(terms, call[1])[0])
        qa.profile_reset()
        getattr(q, call[0])(terms, *call[1:])
        report[name] = {"k": k, "counts": {key: int(v[0]) for key, v in qa.profile_report().items()
                                          if key.startswith("krylov")}}

    counted("tridiagonal", ("lanczos_tridiagonal", 5))
    counted("ground", ("lanczos_ground_state", 6, False))
    counted("prepare", ("lanczos_ground_state", 4, True))
    counted("prepare_long", ("lanczos_ground_state", kc.CAP + 2, True))
    print("REPORT " + json.dumps(report))
    # the evolution: dim and time come first
    q = kc.sim(ENGINE, PROFILE_N, "fp32")
    q.set_state_vector(psi)
    qa.profile_reset()
    q.krylov_evolve_pauli_sum(terms, 0.2, 2 * kc.CAP + 2, 2)
    print("EVOLVE " + json.dumps({key: int(v[0]) for key, v in qa.profile_report().items()
                                  if key.startswith("krylov")}))


@pytest.fixture(scope="module")
def profile_report():
    out = run_child("child_profile", {"QRACK_PROFILE": "1"})
    rep = json.loads([l for l in out.splitlines() if l.startswith("REPORT ")][-1][len("REPORT "):])
    rep["evolve"] = json.loads([l for l in out.splitlines() if l.startswith("EVOLVE ")][-1][len("EVOLVE "):])
    return rep


def test_profile_counts_the_launches(profile_report):
    """k L apply launches and k finishes per run; the combine only where a
    state is built, in the launches the exposed cap implies"""
    launches = ao.launches(kc.chain_terms(PROFILE_N))
    assert launches >= 3

    def want(k, combine):
        counts = {"krylov_apply": k * launches, "krylov_finish": k}
        if combine:
            counts["krylov_combine"] = combine
        return counts

    for name, dim, builds in (("tridiagonal", 5, False), ("ground", 6, False), ("prepare", 4, True),
                              ("prepare_long", kc.CAP + 2, True)):
        k = profile_report[name]["k"]
        assert k == dim
        assert profile_report[name]["counts"] == want(k, kc.combine_launches(k) if builds else 0), name
    assert kc.combine_launches(4) == 1 and kc.combine_launches(kc.CAP + 2) == 2
    dim = 2 * kc.CAP + 2
    assert profile_report["evolve"] == want(2 * dim, 2 * kc.combine_launches(dim))
    assert kc.combine_launches(dim) == 3


# stride loops


def child_stride():
    """run under QRACK_GPU_BLOCKS=2: 512 threads for 1024 or more items, so
    every stride loop takes a second trip"""
    for prec in PRECS:
        kc.widths(ENGINE, 9, prec)
        for x in kc.ac.x_masks_12():
            kc.partner_logic(ENGINE, prec, x)
        kc.chunking(ENGINE, prec)
        kc.dims(ENGINE, prec, kc.CAP + 2)
    print("CHILD_OK")


def test_stride_loops_in_child():
    assert "CHILD_OK" in run_child("child_stride", {"QRACK_GPU_BLOCKS": "2"})


# memory peaks

ALLOC_N = 20  # 8 MiB per fp32 state
ALLOC_DIM = 4


def child_alloc(expect):
    """run under QRACK_MAX_ALLOC_MB at 20 qubits fp32: `expect` says whether
    the cap admits the dim + 1 states of the evolution"""
    q = kc.sim(ENGINE, ALLOC_N, "fp32")
    for b in range(ALLOC_N):
        q.ry(0.3 + 0.05 * b, b)
        q.rz(0.2 + 0.03 * b, b)
    terms = kc.chain_terms(ALLOC_N)
    before = kc.state_of(q)
    a, b = q.lanczos_tridiagonal(terms, 32)
    assert len(a) == 32 and np.all(np.isfinite(a)) and np.all(b > 0)
    print("TRIDIAGONAL_FITS")
    norm0 = float(np.linalg.norm(before.astype(np.complex128)))
    try:
        est = q.krylov_evolve_pauli_sum(terms, 0.05, ALLOC_DIM)
        fitted = True
    except Exception:
        fitted = False
    assert fitted == (expect == "fits")
    after = kc.state_of(q)
    if fitted:
        drift = abs(float(np.linalg.norm(after.astype(np.complex128))) - norm0)
        assert drift <= 16 * ALLOC_DIM * kc.EPS["fp32"] * norm0
        assert 0 < est < 1 and after.tobytes() != before.tobytes()
        print("EVOLVE_FITS")
    else:
        assert after.tobytes() == before.tobytes()
        print("EVOLVE_REFUSED_STATE_INTACT")


def test_evolution_peaks_at_dim_plus_one_states():
    """40 MiB hold the state and the dim = 4 buffers; 39 MiB are one state short"""
    out = run_child("child_alloc", {"QRACK_MAX_ALLOC_MB": "40"}, "fits")
    assert "TRIDIAGONAL_FITS" in out and "EVOLVE_FITS" in out, out
    out = run_child("child_alloc", {"QRACK_MAX_ALLOC_MB": "39"}, "refused")
    assert "EVOLVE_REFUSED_STATE_INTACT" in out, out


def test_tridiagonal_peaks_at_four_states():
    """32 MiB hold four states: lanczos_tridiagonal(dim=32) passes, the evolution does not"""
    out = run_child("child_alloc", {"QRACK_MAX_ALLOC_MB": "32"}, "refused")
    assert "TRIDIAGONAL_FITS" in out and "EVOLVE_REFUSED_STATE_INTACT" in out, out
