"""pauli_sum_braket, pauli_sum_apply_into and adjoint_gradient on the HIP
engine: the pair walk of the Pauli-sum kernels over two vectors, H|psi> into a
second state, and the fused backward step (one launch per trainable rotation).

Oracle and tolerances: adjoint_oracle.py (numpy float64 on the engine's own
get_state_vector()); the checks shared with the CPU engine's file are in
adjoint_cases.py. The child processes pin what only a fresh process can: the
launch counts under QRACK_PROFILE, the stride loops under QRACK_GPU_BLOCKS and
the two-state peak under QRACK_MAX_ALLOC_MB.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po
import adjoint_oracle as ao
import adjoint_cases as ac

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ENGINE = "hip"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ac.PRECS
N12 = ac.N12


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    """One vector or fewer (1, 2), fewer pairs than a wave (5), several blocks (9)."""
    ac.widths(ENGINE, n, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("x", ac.x_masks_12(), ids=lambda x: "x%03x" % x)
def test_partner_logic_12(x, prec):
    """x = 0, bit 0 (in-vector swap), top bit, both, all bits, and single bits
    5-8 (lane, wave and block boundaries of the pair stream)."""
    ac.partner_logic(ENGINE, prec, x)


@pytest.mark.parametrize("prec", PRECS)
def test_conjugation_and_aliasing(prec):
    ac.conjugation_and_aliasing(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_group_larger_than_cap_splits(prec):
    ac.chunking(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_read_only_and_write_all(prec):
    ac.readonly_and_writeall(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_pending_basis_state(prec):
    ac.pending_basis_state(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_bra_on_another_engine_is_staged(prec):
    """a bra that is no HIP engine goes through a host copy, as in sum_sqr_diff"""
    n = 9
    rng = np.random.default_rng(940)
    terms = po.random_terms(n, rng, 20) + [(0.7, [], [])]
    q, psi = ac.sim_with_state("hip", n, prec, 941)
    b, phi = ac.sim_with_state("cpu", n, prec, 942)
    ac.check_braket(b, phi, q, psi, terms, prec, "cpu bra")
    with pytest.raises(Exception):
        q.pauli_sum_apply_into(terms, b)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (5, 9))
def test_gradient(n, prec):
    ac.gradient(ENGINE, n, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_gradient_edges(prec):
    ac.gradient_edges(ENGINE, prec)


@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "hip"]), ids=lambda l: "-".join(l))
def test_layers_reach_engine(layers):
    # fp32 state tolerance of the GPU suite, per unit sum|c|
    ac.layers_match_engine(ENGINE, layers, "fp32", 2e-4)


# ---- child processes ------------------------------------------------------------------


def run_child(fn, env, *args):
    code = ("import os, sys\n"
            "sys.path.insert(0, sys.argv[1])\n"
            "sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
            "import test_adjoint_gpu as t\n"
            f"t.{fn}(*sys.argv[2:])\n")
    r = subprocess.run(
        [sys.executable, "-c", code, ROOT, *args],
        env={**os.environ, **env}, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, f"stdout={r.stdout}\nstderr={r.stderr}"
    return r.stdout


# 8. launch counts

N_ROT, N_TRAIN = 10, 7


def profile_ops():
    """rotations only, N_TRAIN of N_ROT trainable, none an identity string"""
    top = N12 - 1
    ops = [
        ("rot", [0], [1], 0.3),
        ("rot", [top], [3], -0.2),
        ("rot", [0, top], [3, 1], 0.5, False),
        ("rot", [2, 7], [2, 2], 0.4),           # diagonal
        ("rot", [5, 6, 7, 8], [1, 3, 1, 3], -0.6),
        ("rot", [3], [2], 0.1, False),          # diagonal, untrainable
        ("rot", list(range(N12)), [1] * N12, 0.25),
        ("rot", [1, 4], [3, 3], 0.35),
        ("rot", [9, 0], [1, 2], -0.45, False),
        ("rot", [6], [3], 0.15),
    ]
    assert len(ops) == N_ROT and sum(1 for op in ops if len(op) == 4) == N_TRAIN
    return ops


def profile_terms():
    rng = np.random.default_rng(88)
    return ac.terms_sharing_x(0b1001, qa.PAULI_MAX_TERMS + 1, rng) + po.random_terms(N12, rng, 20) \
        + [(0.5, [], [])]


def child_profile():
    """run under QRACK_PROFILE=1 (and with the hybrid layer on the GPU from 12
    qubits on): launch counts of one gradient per stack, as JSON"""
    ops, terms = profile_ops(), profile_terms()
    report = {}
    for name, kw in (("hip", dict(engine="hip")), ("hybrid", dict(layers=["hybrid"]))):
        q = qa.create_simulator(N12, seed=3, **kw)
        q.set_state_vector(po.random_state(N12, np.random.default_rng(89), np.complex64))
        psi0 = np.asarray(q.get_state_vector())
        qa.profile_reset()
        e, g = q.adjoint_gradient(ops, terms)
        rep = qa.profile_report()
        want_e, want_g = ao.gradient(psi0, ops, terms)
        err = max([abs(e - want_e)] + [abs(a - b) for a, b in zip(g, want_g)])
        report[name] = {"counts": {k: int(v[0]) for k, v in rep.items()},
                        "err_over_bound": err / ao.gradient_bound(ops, terms, "fp32")}
    print("REPORT " + json.dumps(report))


@pytest.fixture(scope="module")
def profile_report():
    out = run_child("child_profile", {"QRACK_PROFILE": "1", "QRACK_GPU_THRESHOLD_QB": str(N12)})
    line = [l for l in out.splitlines() if l.startswith("REPORT ")][-1]
    return json.loads(line[len("REPORT "):])


@pytest.mark.parametrize("stack", ("hip", "hybrid"))
def test_profile_counts_the_launches(profile_report, stack):
    """N forward rotations and two launches per untrainable one on the way
    back, L launches of H, one braket for the energy, one fused launch per
    trainable rotation, and nothing else"""
    launches = ao.launches(profile_terms())
    assert launches >= 3
    assert profile_report[stack]["counts"] == {
        "pauli_evolve": N_ROT + 2 * (N_ROT - N_TRAIN),
        "pauli_apply": launches,
        "pauli_braket": 1,
        "pauli_adjoint": N_TRAIN,
    }
    assert profile_report[stack]["err_over_bound"] <= 1.0


# 9. stride loops


def child_stride():
    """run under QRACK_GPU_BLOCKS=2: 512 threads for 1024 or more items, so
    every stride loop takes a second trip"""
    for prec in PRECS:
        ac.partner_logic(ENGINE, prec, 1 | (1 << (N12 - 1)))
        ac.partner_logic(ENGINE, prec, 0)
        ac.chunking(ENGINE, prec)
        ac.gradient(ENGINE, N12, prec)
    print("CHILD_OK")


def test_stride_loops_in_child():
    assert "CHILD_OK" in run_child("child_stride", {"QRACK_GPU_BLOCKS": "2"})


# 10. two states at the peak


def rot3(axis, angle):
    """rotation of a Bloch vector about X (1), Y (3) or Z (2), and its derivative in the angle"""
    k = {1: np.array([1.0, 0, 0]), 3: np.array([0, 1.0, 0]), 2: np.array([0, 0, 1.0])}[axis]
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    kk = np.outer(k, k)
    r = math.cos(angle) * np.eye(3) + math.sin(angle) * kx + (1 - math.cos(angle)) * kk
    dr = -math.sin(angle) * np.eye(3) + math.cos(angle) * kx + math.sin(angle) * kk
    return r, dr


def child_two_states():
    """run under QRACK_MAX_ALLOC_MB=80 at 22 qubits fp32 (32 MiB per state):
    a gradient over 4 rotations on a product state against its closed form,
    then two clones, of which the second must be refused"""
    n = 22
    comp = {1: 0, 3: 1, 2: 2}
    q = qa.create_simulator(n, engine="hip", precision="fp32", seed=2)
    bloch = []
    for b in range(n):
        theta, phi = 0.4 + 0.05 * b, 0.3 + 0.07 * b
        q.ry(theta, b)
        q.rz(phi, b)
        bloch.append(np.array([math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi),
                               math.cos(theta)]))
    # exp(-i alpha P) turns the Bloch vector by 2 alpha about P's axis
    rots = [(0, 1, 0.3), (n - 1, 3, -0.4), (10, 2, 0.5), (0, 2, 0.2)]
    ops = [("rot", [b], [p], a) for b, p, a in rots]
    terms = [(1.0, [0], [3]), (0.7, [n - 1], [1]), (0.5, [10], [1]), (0.8, [0, n - 1], [2, 1]),
             (0.6, [5], [2]), (0.4, [5, 10, 0], [1, 3, 1]), (0.3, [], [])]

    def vectors(deriv=None):
        v = [b.copy() for b in bloch]
        for k, (b, p, a) in enumerate(rots):
            r, dr = rot3(p, 2 * a)
            v[b] = (2 * dr if k == deriv else r) @ v[b]
        return v

    def energy(v, dv=None, which=None):
        total = 0.0
        for c, qs, ps in terms:
            if dv is None:
                total += c * math.prod(v[b][comp[p]] for b, p in zip(qs, ps))
            elif which in qs:
                total += c * math.prod((dv if b == which else v)[b][comp[p]] for b, p in zip(qs, ps))
        return total

    want_e = energy(vectors())
    want_g = [energy(vectors(), vectors(k), rots[k][0]) for k in range(len(rots))]
    e, g = q.adjoint_gradient(ops, terms)
    tol = 2e-4 * po.abs_coeffs(terms)
    assert abs(e - want_e) <= tol, (e, want_e)
    assert all(abs(a - b) <= 2 * tol for a, b in zip(g, want_g)), (list(g), want_g)
    assert max(abs(x) for x in want_g) > 0.1
    print("GRADIENT_OK")
    first = q.clone()
    print("FIRST_CLONE_FITS")
    try:
        second = q.clone()
        print("SECOND_CLONE_FITS")
    except Exception:
        print("SECOND_CLONE_REFUSED")


def test_gradient_peaks_at_two_states():
    """the cap admits two states and refuses a third: the gradient needs two"""
    r = subprocess.run(
        [sys.executable, "-c",
         "import os, sys\nsys.path.insert(0, sys.argv[1])\n"
         "sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
         "import test_adjoint_gpu as t\nt.child_two_states()\n", ROOT],
        env={**os.environ, "QRACK_MAX_ALLOC_MB": "80"}, capture_output=True, text=True, timeout=300,
    )
    out = r.stdout
    assert "GRADIENT_OK" in out, f"stdout={out}\nstderr={r.stderr}"
    assert "FIRST_CLONE_FITS" in out, f"stdout={out}\nstderr={r.stderr}"
    assert "SECOND_CLONE_REFUSED" in out, f"the cap does not bite: stdout={out}\nstderr={r.stderr}"
