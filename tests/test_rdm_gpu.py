"""Multi-qubit reduced density matrices on the HIP engine: the register, tile
and wide regimes of rdm_pass_plan, read-only, no clone, no scratch.

Oracle and tolerance: rdm_oracle.py, on the engine's own get_state_vector().
E_R = qa.RDM_RUN is the longest run the tile kernel sums in the engine's real
type (asserted <= 64); the register kernel sums in double throughout and is
held to the same bound.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import rdm_oracle as ro

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("fp32", "fp64")
N12 = 12
E_R = qa.RDM_RUN


def hip_with_state(n, prec, seed):
    rng = np.random.default_rng(seed)
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=1)
    q.set_state_vector(ro.random_state(n, rng, ro.DTYPE[prec]))
    return q, np.asarray(q.get_state_vector())


def check_call(q, sv, kept, prec):
    """Everything a call must satisfy: Hermitian to the bit, the elementwise
    bound, the trace, a bit-identical repeat, an untouched state."""
    assert E_R <= 64
    want = ro.rdm(sv, kept)
    got = q.reduced_density_matrix(kept)
    ro.check(got, want, prec, E_R, kept)
    D = 1 << len(kept)
    norm = float(np.sum(np.abs(sv.astype(np.complex128)) ** 2))
    assert abs(got.trace().real - norm) <= D * (4 + E_R) * ro.EPS[prec], kept
    assert got.tobytes() == q.reduced_density_matrix(kept).tobytes(), kept
    assert np.asarray(q.get_state_vector()).tobytes() == sv.tobytes(), kept
    return got


@pytest.fixture(scope="module", params=PRECS)
def state12(request):
    """One random 12-qubit state per precision, downloaded once, never changed."""
    q, sv = hip_with_state(N12, request.param, 1212)
    return request.param, q, sv


# ---- 1. small widths -----------------------------------------------------------------


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    """Fewer rows than a wave, fewer than a block, several blocks; k = n has
    no environment at all."""
    q, sv = hip_with_state(n, prec, 500 + n)
    for b in sorted({0, n // 2, n - 1}):
        check_call(q, sv, [b], prec)
    check_call(q, sv, list(range(n)), prec)
    check_call(q, sv, list(range(n))[::-1], prec)


# ---- 2. every compile-time k, both sides of the register / tile boundary -------------


def kept_sets(k):
    low = list(range(k))
    high = list(range(N12 - k, N12))
    inner = [1, 3, 5, 7, 9, 2, 4, 6, 8, 10][:max(k - 2, 0)]
    scattered = sorted([0, N12 - 1] + inner) if k > 1 else [0]
    unsorted = [(7 * j + 5) % N12 for j in range(k)]
    assert len(set(unsorted)) == k and unsorted != sorted(unsorted) or k == 1
    return {"low": low, "high": high, "scattered": scattered, "unsorted": unsorted}


@pytest.mark.parametrize("which", ("low", "high", "scattered", "unsorted"))
@pytest.mark.parametrize("k", range(1, 7))
def test_register_and_tile_regimes(state12, k, which):
    prec, q, sv = state12
    kept = kept_sets(k)[which]
    plan = qa.rdm_pass_plan(N12, kept, prec)
    assert plan["regime"] == ("register" if k <= qa.RDM_REG_MAX else "tile")
    check_call(q, sv, kept, prec)


def test_order_is_honoured(state12):
    prec, q, sv = state12
    a = q.reduced_density_matrix([7, 2, 11])
    b = q.reduced_density_matrix([2, 7, 11])
    perm = [((i & 1) << 1) | ((i >> 1) & 1) | (i & 4) for i in range(8)]
    assert not np.array_equal(a, b) and np.array_equal(a, b[np.ix_(perm, perm)])


# ---- 3. wide regime ---------------------------------------------------------------------


@pytest.mark.parametrize("which", ("low", "high", "scattered"))
@pytest.mark.parametrize("k", (7, 8))
def test_wide_regime(state12, k, which):
    prec, q, sv = state12
    kept = kept_sets(k)[which]
    plan = qa.rdm_pass_plan(N12, kept, prec)
    assert plan["regime"] == "wide" and len(plan["launches"]) == {7: 3, 8: 10}[k]
    check_call(q, sv, kept, prec)


@pytest.mark.parametrize("k", (11, 12))
def test_wide_regime_little_or_no_environment(state12, k):
    prec, q, sv = state12
    kept = [b for b in range(N12) if k == 12 or b != 4]
    got = check_call(q, sv, kept, prec)
    if k == 12:
        v = sv.astype(np.complex128)
        assert np.all(np.abs(got - np.outer(v, v.conj())) <= ro.bound(got, prec, E_R))


# ---- 4. every stride loop takes a second trip --------------------------------------------

_CHILD_BLOCKS = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import qrack_amd as qa
import rdm_oracle as ro
n = 14
for prec in ("fp32", "fp64"):
    rng = np.random.default_rng(1400)
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=1)
    q.set_state_vector(ro.random_state(n, rng, ro.DTYPE[prec]))
    sv = np.asarray(q.get_state_vector())
    for kept in ([13, 0], [3, 9], [12, 1, 6, 0, 8], [2, 13, 5, 7, 10, 3, 11], [0, 1, 2, 3, 4, 5, 6, 7]):
        got = q.reduced_density_matrix(kept)
        ro.check(got, ro.rdm(sv, kept), prec, qa.RDM_RUN, kept)
        assert got.tobytes() == q.reduced_density_matrix(kept).tobytes()
    print("OK", prec)
"""


def test_two_blocks_in_a_fresh_process():
    r = subprocess.run(
        [sys.executable, "-c", _CHILD_BLOCKS, ROOT],
        env={**os.environ, "QRACK_GPU_BLOCKS": "2"},
        capture_output=True, text=True, timeout=300,
    )
    assert "OK fp32" in r.stdout and "OK fp64" in r.stdout, f"stdout={r.stdout}\nstderr={r.stderr}"


# ---- 5. grid stride at the full grid -------------------------------------------------------


def test_grid_stride_product_state():
    """24 qubits: 2^22 rows (k = 2) exceed the register grid's 2^19 threads
    and 2^12 tiles (k = 5) the tile grid's 2^10 blocks."""
    n = 24
    q = qa.create_simulator(n, engine="hip", precision="fp32", seed=2)
    one = []
    for b in range(n):
        theta, phi = 0.3 + 0.1 * b, 0.2 + 0.05 * b
        q.ry(theta, b)
        q.rz(phi, b)
        # rz(phi) ry(theta) |0> = (cos(theta/2), e^{i phi} sin(theta/2)) up to a phase
        v = np.array([math.cos(theta / 2), np.exp(1j * phi) * math.sin(theta / 2)])
        one.append(np.outer(v, v.conj()))
    for kept in ([23, 0], [1, 22, 0, 13, 23]):
        want = np.ones((1, 1), dtype=np.complex128)
        for b in kept:  # qubits[0] is the lowest index bit: the last Kronecker factor
            want = np.kron(one[b], want)
        got = q.reduced_density_matrix(kept)
        assert np.array_equal(got, got.conj().T)
        assert np.abs(got - want).max() <= 2e-4, kept


# ---- 6. read-only: pending basis state, tile sums -------------------------------------------


@pytest.mark.parametrize("prec", PRECS)
def test_pending_basis_state(prec):
    n, p, kept = 10, 0x2A5, [1, 8, 3]
    a = sum(((p >> b) & 1) << j for j, b in enumerate(kept))
    want = np.zeros((8, 8), dtype=np.complex128)
    want[a, a] = 1.0
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=4)
    q.set_permutation(p)
    assert np.array_equal(q.reduced_density_matrix(kept), want)
    q.h(1)  # leave something else in the buffer
    q.set_permutation(p)
    assert np.array_equal(q.reduced_density_matrix(kept), want)
    assert np.array_equal(q.reduced_density_matrix(list(range(7))).nonzero()[0], [p & 0x7F])


def test_tile_sums_survive_an_rdm_call():
    """QFT leaves per-tile norms for the sampler; a reduced density matrix in
    between reads the state only, so sampling matches an engine that never
    made the call."""
    n = 23
    pows = [1 << i for i in range(n)]

    def prepared():
        q = qa.create_simulator(n, engine="hip", seed=21)
        q.set_permutation(5)
        for i in range(0, n, 4):
            q.ry(0.9 + 0.05 * i, i)
        q.qft(0, n)
        return q

    a, b = prepared(), prepared()
    for kept in ([0, 22], [3, 9, 1, 20, 14]):
        rho = a.reduced_density_matrix(kept)
        assert abs(rho.trace().real - 1.0) <= 2e-4
    shots_a = a.multi_shot_measure_mask(pows, 64)
    shots_b = b.multi_shot_measure_mask(pows, 64)
    assert sum(shots_a.values()) == 64
    assert shots_a == shots_b


# ---- 7. no clone, no scratch ------------------------------------------------------------------

_CHILD_CAP = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import qrack_amd as qa
n = 22
q = qa.create_simulator(n, engine="hip", precision="fp32", seed=1)
q.h(0)
q.cnot(0, 21)
q.h(5)
assert abs(q.prob(0) - 0.5) < 1e-5
print("GATE_OK")
try:
    q.clone()
    print("CLONE_FITS")
except Exception:
    print("CLONE_REFUSED")
# (|00> + |11>)/sqrt(2) on qubits 0 and 21, |+> on qubit 5
bell = np.zeros((4, 4)); bell[0, 0] = bell[0, 3] = bell[3, 0] = bell[3, 3] = 0.5
assert np.abs(q.reduced_density_matrix([0, 21]) - bell).max() < 2e-4
print("PAIR_OK")
assert np.abs(q.reduced_density_matrix([5]) - np.full((2, 2), 0.5)).max() < 2e-4
assert np.abs(np.asarray(q.reduced_density_matrix(5)) - np.full((2, 2), 0.5)).max() < 2e-4
print("ONE_OK")
"""


def test_no_clone_no_scratch_under_alloc_cap():
    """A 22-qubit fp32 state is 32 MiB; under a 48 MiB cap one state fits and
    a clone or a scratch buffer does not."""
    r = subprocess.run(
        [sys.executable, "-c", _CHILD_CAP, ROOT],
        env={**os.environ, "QRACK_MAX_ALLOC_MB": "48"},
        capture_output=True, text=True, timeout=300,
    )
    out = r.stdout
    assert "GATE_OK" in out, f"stdout={out}\nstderr={r.stderr}"
    assert "CLONE_REFUSED" in out, f"the cap does not bite: stdout={out}\nstderr={r.stderr}"
    assert "PAIR_OK" in out and "ONE_OK" in out, f"stdout={out}\nstderr={r.stderr}"


# ---- 8. through layers ---------------------------------------------------------------------------


@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "hip"]), ids=lambda l: "-".join(l))
def test_layers_reach_engine(layers):
    n = N12

    def circuit(q):
        for i in range(n):
            q.ry(0.2 + 0.3 * i, i)
        for i in range(n - 1):
            q.cnot(i, i + 1)
        for i in range(n):
            q.rz(0.15 * (i + 1), i)
        return q

    bare = circuit(qa.create_simulator(n, engine="hip", seed=3))
    q = circuit(qa.create_simulator(n, layers=layers, seed=3))
    tol = 2e-4  # fp32 state tolerance of the GPU suite: gate rounding is included
    before = np.asarray(q.get_state_vector()).tobytes()
    for kept in ([11, 0], [6, 2, 9, 0, 4], [1, 3, 5, 7, 8, 9, 10]):
        got = q.reduced_density_matrix(kept)
        assert np.abs(got - bare.reduced_density_matrix(kept)).max() <= tol, kept
    one = np.asarray(q.reduced_density_matrix(0)).astype(np.complex128)
    assert np.abs(one - q.reduced_density_matrix([0])).max() <= 2 * ro.EPS["fp32"]
    assert np.asarray(q.get_state_vector()).tobytes() == before
