"""Pauli-string and Pauli-sum expectation values on the HIP engine: one
read-only pass per X/Y mask, no clone, no scratch, one host sync per call.

Oracle: numpy float64 dense index arithmetic on the engine's own
get_state_vector() (isolates the kernels from gate rounding). Tolerance on
|got - want| is 1e-6 * sum|c_t| (fp32) and 1e-12 * sum|c_t| (fp64): the
half-space products satisfy sum 2|psi_i||psi_j| <= 1 and each carries a few
ulp of the amplitude type (about 2.4e-7 for fp32); the sum is in double.
"""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"fp32": 1e-6, "fp64": 1e-12}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}
PRECS = ("fp32", "fp64")
N12 = 12


def hip_with_state(n, prec, seed):
    rng = np.random.default_rng(seed)
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=1)
    q.set_state_vector(po.random_state(n, rng, DTYPE[prec]))
    return q, np.asarray(q.get_state_vector()), rng


@pytest.fixture(scope="module", params=PRECS)
def state12(request):
    """One random 12-qubit state per precision, downloaded once, never changed."""
    q, sv, _ = hip_with_state(N12, request.param, 1200)
    return request.param, q, sv


def check_strings(q, sv, strings, tol):
    for qs, ps in strings:
        want = po.expect(sv, qs, ps)
        assert abs(q.pauli_expectation(qs, ps) - want) <= tol, (qs, ps)
        assert abs(q.expectation_pauli_all(qs, ps) - want) <= tol, (qs, ps)
        # d(1 - E^2) = 2|E| dE <= 2 dE
        assert abs(q.variance_pauli_all(qs, ps) - (1 - want * want)) <= 2 * tol, (qs, ps)


# ---- 1. index and partner logic ----------------------------------------------


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    """Fewer pairs than a wave (1, 2, 5), fewer than a block and several blocks (9)."""
    q, sv, rng = hip_with_state(n, prec, 300 + n)
    if n <= 2:
        strings = [(list(range(n)), list(ps)) for ps in itertools.product(range(4), repeat=n)]
    else:
        strings = [po.random_string(n, rng) for _ in range(64)]
    check_strings(q, sv, strings, TOL[prec])
    terms = po.random_terms(n, rng, 40)
    got = q.expectation_pauli_sum(terms)
    assert abs(got - po.expect_sum(sv, terms)) <= TOL[prec] * po.abs_coeffs(terms)


def x_masks_12():
    top = 1 << (N12 - 1)
    return [1, top, 1 | top, (1 << N12) - 1] + [1 << b for b in (5, 6, 7, 8)]


def strings_for_mask(x):
    """x crossed with ny mod 4, Z factors below/above the top x bit, Y on the top x bit."""
    xbits = [b for b in range(N12) if (x >> b) & 1]
    top = xbits[-1]
    free = [b for b in range(N12) if not (x >> b) & 1]
    below = [b for b in free if b < top][-1:]
    above = [b for b in free if b > top][:1]
    z_sets = [[], below, above, below + above]
    out = []
    for ny in range(min(4, len(xbits)) + 1):
        placements = {tuple(xbits[len(xbits) - ny:])}  # Y on the top x bits
        placements.add(tuple(xbits[:ny]))               # Y on the low x bits, X on top
        for ybits in placements:
            for zs in z_sets:
                qs = xbits + zs
                ps = [3 if b in ybits else 1 for b in xbits] + [2] * len(zs)
                out.append((qs, ps))
    return out


@pytest.mark.parametrize("x", x_masks_12(), ids=lambda x: "x%03x" % x)
def test_partner_logic_12(state12, x):
    """bit 0 (in-vector swap), top bit, both, all bits, and single bits 5-8
    (lane, wave and block boundaries of the pair stream)."""
    prec, q, sv = state12
    strings = strings_for_mask(x)
    assert {po.masks(qs, ps)[0] for qs, ps in strings} == {x}
    assert len({po.masks(qs, ps)[2] % 4 for qs, ps in strings}) == min(4, bin(x).count("1") + 1)
    check_strings(q, sv, strings, TOL[prec])
    rng = np.random.default_rng(x)
    terms = [(float(rng.uniform(-1, 1)), qs, ps) for qs, ps in strings]
    got = q.expectation_pauli_sum(terms)
    assert abs(got - po.expect_sum(sv, terms)) <= TOL[prec] * po.abs_coeffs(terms)


# ---- 2. grouping ---------------------------------------------------------------


def terms_sharing_x(x, count, rng):
    """count distinct strings with the same X/Y mask: z runs over distinct masks."""
    xbits = [b for b in range(N12) if (x >> b) & 1]
    zs = rng.choice(1 << N12, size=count, replace=False)
    terms = []
    for z in zs:
        qs, ps = [], []
        for b in range(N12):
            code = (1 if b in xbits else 0) | (2 if (int(z) >> b) & 1 else 0)
            if code:
                qs.append(b)
                ps.append(code)
        terms.append((float(rng.uniform(-1, 1)), qs, ps))
    return terms


def test_group_larger_than_cap_splits(state12):
    prec, q, sv = state12
    assert qa.PAULI_MAX_TERMS >= 1
    rng = np.random.default_rng(77)
    x = (1 << 1) | (1 << 4) | (1 << 9)
    terms = terms_sharing_x(x, qa.PAULI_MAX_TERMS + 3, rng)
    assert {po.masks(qs, ps)[0] for _, qs, ps in terms} == {x}
    tol = TOL[prec] * po.abs_coeffs(terms)
    got = q.expectation_pauli_sum(terms)
    per_term = sum(c * q.pauli_expectation(qs, ps) for c, qs, ps in terms)
    assert abs(got - per_term) <= tol
    assert abs(got - po.expect_sum(sv, terms)) <= tol


def test_mixed_sum_and_repeatability(state12):
    prec, q, sv = state12
    rng = np.random.default_rng(78)
    xs = [0] + [int(v) for v in rng.choice(np.arange(1, 1 << N12), size=9, replace=False)]
    terms = []
    for x in xs:
        terms += terms_sharing_x(x, 10, rng)
    assert len(terms) == 100 and len({po.masks(qs, ps)[0] for _, qs, ps in terms}) == 10
    order = rng.permutation(len(terms))
    terms = [terms[i] for i in order]
    a = q.expectation_pauli_sum(terms)
    b = q.expectation_pauli_sum(terms)
    assert a == b  # fixed reduction order: bit-identical
    assert abs(a - po.expect_sum(sv, terms)) <= TOL[prec] * po.abs_coeffs(terms)


# ---- 3. read-only, lazy basis state, tile sums ---------------------------------


def test_state_is_untouched(state12):
    prec, q, sv = state12
    before = sv.tobytes()
    rng = np.random.default_rng(79)
    qs, ps = [3, 0, 11, 7], [1, 3, 2, 3]
    terms = po.random_terms(N12, rng, 30)
    for call in (
        lambda: q.pauli_expectation(qs, ps),
        lambda: q.expectation_pauli_all(qs, ps),
        lambda: q.variance_pauli_all(qs, ps),
        lambda: q.expectation_pauli_sum(terms),
    ):
        call()
        assert np.asarray(q.get_state_vector()).tobytes() == before


@pytest.mark.parametrize("prec", PRECS)
def test_pending_basis_state(prec):
    n, p = 10, 0x2A5
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=4)
    q.h(1)  # leave something else in the buffer first
    rng = np.random.default_rng(5)
    for _ in range(8):
        qs, ps = po.random_string(n, rng)
        x, z, _ = po.masks(qs, ps)
        want = 0.0 if x else float(1 - 2 * (bin(p & z).count("1") & 1))
        q.set_permutation(p)
        assert q.pauli_expectation(qs, ps) == want, (qs, ps)
        q.set_permutation(p)
        assert q.expectation_pauli_sum([(0.5, qs, ps)]) == 0.5 * want, (qs, ps)


def test_tile_sums_survive_pauli_sum():
    """QFT leaves per-tile norms for the sampler; a Pauli sum in between reads
    the state only, so sampling matches an engine that never made the call."""
    n = 23
    pows = [1 << i for i in range(n)]

    def prepared():
        q = qa.create_simulator(n, engine="hip", seed=21)
        q.set_permutation(5)
        for i in range(0, n, 4):
            q.ry(0.9 + 0.05 * i, i)
        q.qft(0, n)
        return q

    terms = [(1.0, [b], [2]) for b in range(n)] + [(0.5, [0, n - 1], [1, 3])]
    a, b = prepared(), prepared()
    e = a.expectation_pauli_sum(terms)
    assert e == a.expectation_pauli_sum(terms)
    per_term = sum(c * b.pauli_expectation(qs, ps) for c, qs, ps in terms[-1:])
    per_term += sum(1 - 2 * b.prob(qs[0]) for _, qs, _ in terms[:-1])
    assert abs(e - per_term) <= 2e-4 * po.abs_coeffs(terms)
    shots_a = a.multi_shot_measure_mask(pows, 64)
    shots_b = b.multi_shot_measure_mask(pows, 64)
    assert sum(shots_a.values()) == 64
    assert shots_a == shots_b


# ---- 4. no clone, no scratch -----------------------------------------------------

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import qrack_amd as qa
n = 22
q = qa.create_simulator(n, engine="hip", precision="fp32", seed=1)
q.h(0)
q.h(1)
q.s(1)
assert abs(q.prob(0) - 0.5) < 1e-5
print("GATE_OK")
try:
    q.clone()
    print("CLONE_FITS")
except Exception:
    print("CLONE_REFUSED")
# |+>|+i>|0>...: <X0 Y1 Z2> = 1
e = q.expectation_pauli_all([0, 1, 2], [1, 3, 2])
assert abs(e - 1.0) < 2e-4, e
print("ALL_OK")
s = q.expectation_pauli_sum([(0.5, [0, 1, 2], [1, 3, 2]), (0.25, [0], [1]), (2.0, [2, 5], [2, 2])])
assert abs(s - 2.75) < 2e-4 * 2.75, s
print("SUM_OK")
"""


def test_no_clone_no_scratch_under_alloc_cap():
    """A 22-qubit fp32 state is 32 MiB; under a 48 MiB cap one state fits and
    a clone or a scratch buffer does not."""
    r = subprocess.run(
        [sys.executable, "-c", _CHILD, ROOT],
        env={**os.environ, "QRACK_MAX_ALLOC_MB": "48"},
        capture_output=True, text=True, timeout=300,
    )
    out = r.stdout
    assert "GATE_OK" in out, f"stdout={out}\nstderr={r.stderr}"
    assert "CLONE_REFUSED" in out, f"the cap does not bite: stdout={out}\nstderr={r.stderr}"
    assert "ALL_OK" in out and "SUM_OK" in out, f"stdout={out}\nstderr={r.stderr}"


# ---- 5. grid-stride range ----------------------------------------------------------


def bloch(code, theta, phi):
    return {1: math.sin(theta) * math.cos(phi), 3: math.sin(theta) * math.sin(phi),
            2: math.cos(theta)}[code]


# 25 qubits: the half-space (2^24 pairs) exceeds the reduction grid's 2^23
# threads, so the one-pair-per-thread streams (x == 1, diagonal) grid-stride.
# 26 qubits: the fp32 two-pairs-per-thread stream does too.
@pytest.mark.parametrize("n", (25, 26))
def test_grid_stride_product_state(n):
    codes = [(1, 3, 2)[b % 3] for b in range(n)]  # mixed X/Y/Z over every qubit
    codes[n - 1] = 3
    angles = []
    q = qa.create_simulator(n, engine="hip", precision="fp32", seed=2)
    for b, c in enumerate(codes):
        # aim each qubit near its own Pauli's +1 eigenstate so that the
        # weight-n product stays far from zero
        d = 0.1 + 0.004 * b
        theta = d if c == 2 else math.pi / 2 - d
        phi = math.pi / 2 - d if c == 3 else d
        q.ry(theta, b)
        q.rz(phi, b)
        angles.append((theta, phi))
    high_x = max(b for b in range(n - 1) if codes[b] == 1)
    strings = [
        (list(range(n)), codes),
        ([0, 2, 5], [1, 2, 2]),        # x == 1
        ([4, high_x, 8], [3, 1, 2]),
    ]
    for qs, ps in strings:
        want = math.prod(bloch(p, *angles[b]) for b, p in zip(qs, ps))
        assert abs(want) > 0.3
        assert abs(q.pauli_expectation(qs, ps) - want) <= 2e-4, (qs, ps)
    zz = [(1.0, [b, b + 1], [2, 2]) for b in range(n - 1)]  # one diagonal pass
    want = sum(bloch(2, *angles[b]) * bloch(2, *angles[b + 1]) for b in range(n - 1))
    assert abs(q.expectation_pauli_sum(zz) - want) <= 2e-4 * len(zz)


def stride_cases():
    """(x, strings, weighted terms) for x == 0 and every mask of x_masks_12()"""
    diag = [([0], [2]), ([N12 - 1], [2]), ([0, N12 - 1], [2, 2]), ([5, 6, 7, 8], [2] * 4),
            (list(range(N12)), [2] * N12)]
    out = []
    for x in [0] + x_masks_12():
        strings = strings_for_mask(x) if x else diag
        rng = np.random.default_rng(500 + x)
        out.append((x, strings, [(float(rng.uniform(-1, 1)), qs, ps) for qs, ps in strings]))
    return out


def stride_mixed_terms():
    rng = np.random.default_rng(81)
    terms = []
    for x in (0, 1, 0x801, 0x1e0):
        terms += terms_sharing_x(x, 10, rng)
    return [terms[i] for i in rng.permutation(len(terms))]


def child_stride_values(path):
    """run by the child under QRACK_GPU_BLOCKS=2: per string, per group and mixed-sum values"""
    out = {}
    for prec in PRECS:
        q, sv, _ = hip_with_state(N12, prec, 1200)
        out[f"{prec}_sv"] = sv
        for x, strings, terms in stride_cases():
            vals = [q.pauli_expectation(qs, ps) for qs, ps in strings]
            out[f"{prec}_{x}"] = np.array(vals + [q.expectation_pauli_sum(terms)])
        mixed = stride_mixed_terms()
        out[f"{prec}_mixed"] = np.array([q.expectation_pauli_sum(mixed), q.expectation_pauli_sum(mixed)])
    np.savez(path, **out)


_CHILD_STRIDE = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_pauli_sum_gpu as t
t.child_stride_values(sys.argv[2])
print("CHILD_OK")
"""


def test_stride_loop_in_child(tmp_path):
    """QRACK_GPU_BLOCKS=2 (read once per process) leaves 512 threads for the
    1024 items of the fp32 two-pair stream and the 2048 or more of every other
    one, so at 12 qubits each addressing mode takes a second trip."""
    path = str(tmp_path / "values.npz")
    r = subprocess.run(
        [sys.executable, "-c", _CHILD_STRIDE, ROOT, path],
        env={**os.environ, "QRACK_GPU_BLOCKS": "2"}, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, f"stdout={r.stdout}\nstderr={r.stderr}"
    data = np.load(path)
    for prec in PRECS:
        sv = data[f"{prec}_sv"]
        for x, strings, terms in stride_cases():
            vals = data[f"{prec}_{x}"]
            assert len(vals) == len(strings) + 1
            assert {po.masks(qs, ps)[0] for qs, ps in strings} == {x}
            for got, (qs, ps) in zip(vals, strings):
                assert abs(got - po.expect(sv, qs, ps)) <= TOL[prec], (prec, qs, ps)
            assert abs(vals[-1] - po.expect_sum(sv, terms)) <= TOL[prec] * po.abs_coeffs(terms), (prec, x)
        mixed = stride_mixed_terms()
        assert len(mixed) == 40 and len({po.masks(qs, ps)[0] for _, qs, ps in mixed}) == 4
        a, b = data[f"{prec}_mixed"]
        assert a.tobytes() == b.tobytes()  # fixed reduction order: bit-identical
        assert abs(a - po.expect_sum(sv, mixed)) <= TOL[prec] * po.abs_coeffs(mixed), prec


# ---- 6. through layers ---------------------------------------------------------------


@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "hip"]), ids=lambda l: "-".join(l))
def test_layers_reach_engine(layers):
    n = N12
    rng = np.random.default_rng(90)
    terms = po.random_terms(n, rng, 30)
    qs, ps = [2, 11, 0, 6], [3, 1, 2, 3]

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
    assert abs(q.expectation_pauli_sum(terms) - bare.expectation_pauli_sum(terms)) \
        <= tol * po.abs_coeffs(terms)
    before = np.asarray(q.get_state_vector()).tobytes()
    assert abs(q.pauli_expectation(qs, ps) - bare.pauli_expectation(qs, ps)) <= tol
    assert abs(q.expectation_pauli_all(qs, ps) - bare.expectation_pauli_all(qs, ps)) <= tol
    assert abs(q.variance_pauli_all(qs, ps) - bare.variance_pauli_all(qs, ps)) <= 2 * tol
    q.expectation_pauli_sum(terms)
    # the native path reads only; the generic lowering would rotate the state
    assert np.asarray(q.get_state_vector()).tobytes() == before
