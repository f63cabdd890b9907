"""Structural kernels (k_compose, k_allocate_expand, k_dispose_slice,
k_gather_part, k_part_probs) and reductions (k_reduce, k_argmax, k_inner,
k_applym, k_applyparity) of the HIP engine against numpy (alu_oracle.py).

eps_R is 2^-23 (fp32) or 2^-52 (fp64). Inputs are random dense states cast
to the engine's precision; the cast state, promoted to complex128, is the
oracle's input.

Bounds
  compose           8 eps_R max|expected|: one complex product in R.
  allocate, clone   exact.
  dispose_perm, dispose, decompose
                    these divide by the square root of a reduced
                    probability. The same cases on the CPU engine against
                    the oracle gave, as the largest elementwise error in
                    units of eps_R max|expected| (fp32 / fp64):
                      dispose_perm  0.00 / 1.04
                      dispose       1.38 / 2.05
                      decompose     1.55 / 2.13
                    (CPU_DISPOSE_PERM, CPU_DISPOSE, CPU_DECOMPOSE below).
                    The HIP bound is 4x the figure (different summation
                    order of the GPU reductions), floored at 64, so the
                    floor of 64 eps_R max|expected| is what holds here.
  reductions        |got - ref| <= 16 eps_R S, S = sum |value_i| |amp_i|^2
                    (1 for probabilities): <= 3 roundings in R per term,
                    accumulation in double, one final rounding to R.
  collapses         16 eps_R max|expected| on the post-measurement state.
  24 qubits         a product state built with one ry per qubit, never
                    transferred, against closed forms. The gates bound the
                    error, not the reduction: the CPU engine at 16 qubits
                    with the same angles is off by at most 6.66e-8 / 1.76e-16
                    (fp32 / fp64, in units of S; CPU_PRODUCT below); HIP
                    gets 4x that.
"""

import numpy as np
import pytest

import qrack_amd as qa
import alu_oracle as ao

pytestmark = pytest.mark.gpu

EPS = {"fp32": 2.0**-23, "fp64": 2.0**-52}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}
PRECISIONS = ["fp32", "fp64"]

# largest CPU-engine error, in eps_R max|expected|, (fp32, fp64)
CPU_DISPOSE_PERM = {"fp32": 0.00, "fp64": 1.04}
CPU_DISPOSE = {"fp32": 1.38, "fp64": 2.05}
CPU_DECOMPOSE = {"fp32": 1.55, "fp64": 2.13}
# largest CPU-engine error of the 16-qubit product state, in units of S
CPU_PRODUCT = {"fp32": 6.66e-8, "fp64": 1.76e-16}


def sim(n, precision, engine="hip"):
    if engine == "hip":
        assert qa.hip_device_count() > 0, "HIP engine must be present on GPU box (no silent fallback)"
    return qa.create_simulator(n, precision=precision, engine=engine, seed=7)


def cast(state, precision):
    return state.astype(DTYPE[precision]).astype(np.complex128)


def load(state, precision, engine="hip"):
    q = sim(int(state.size).bit_length() - 1, precision, engine)
    q.set_state_vector(state.astype(DTYPE[precision]))
    return q


def read(q):
    return np.asarray(q.get_state_vector()).astype(np.complex128)


def dense(n, seed, precision):
    return cast(ao.random_dense_state(n, np.random.default_rng(seed)), precision)


def max_err(got, expected):
    """Largest elementwise error in units of max|expected|."""
    return float(np.abs(got - expected).max() / np.abs(expected).max())


def structural_bound(cpu_figure, precision):
    return max(4.0 * cpu_figure[precision], 64.0) * EPS[precision]


# ---- compose / allocate / clone --------------------------------------------------


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inserted", [1, 3])
@pytest.mark.parametrize("start", [0, 4, 9])
def test_compose_at(start, inserted, precision):
    a, b = dense(9, 11, precision), dense(inserted, 12, precision)
    qa_, qb = load(a, precision), load(b, precision)
    assert qa_.compose_at(qb, start) == start
    err = max_err(read(qa_), ao.compose(a, b, start))
    print(f"compose_at: {err / EPS[precision]:.2f} eps")
    assert err <= 8 * EPS[precision]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inserted", [1, 3])
def test_compose_at_the_top_and_clone(inserted, precision):
    a, b = dense(9, 13, precision), dense(inserted, 14, precision)
    qa_, qb = load(a, precision), load(b, precision)
    assert qa_.compose(qb) == 9
    got = np.asarray(qa_.get_state_vector())
    err = max_err(got.astype(np.complex128), ao.compose(a, b, 9))
    print(f"compose: {err / EPS[precision]:.2f} eps")
    assert err <= 8 * EPS[precision]
    clone = qa_.clone()
    assert clone.num_qubits == 9 + inserted
    assert np.array_equal(np.asarray(clone.get_state_vector()), got)
    assert np.array_equal(np.asarray(qa_.get_state_vector()), got)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("length", [1, 3])
@pytest.mark.parametrize("start", [0, 4, 9])
def test_allocate(start, length, precision):
    a = dense(9, 15, precision)
    q = load(a, precision)
    assert q.allocate(start, length) == start
    got = np.asarray(q.get_state_vector())
    assert np.array_equal(got, ao.allocate(a, start, length).astype(DTYPE[precision]))


# ---- dispose / decompose ----------------------------------------------------------


def dispose_perm_error(engine, precision):
    """Product of a random 8-qubit state and a 3-qubit basis state."""
    worst = 0.0
    for start, perm in ((4, 5), (8, 6), (1, 3)):
        a = dense(8, 20 + start, precision)
        basis = np.zeros(8, dtype=np.complex128)
        basis[perm] = 1
        q = load(ao.compose(a, basis, start), precision, engine)
        q.dispose_perm(start, 3, perm)
        assert q.num_qubits == 8
        worst = max(worst, max_err(read(q), a))
    return worst


def dispose_error(engine, precision):
    """Product of a random 9-qubit state and a random 2-qubit state. The
    remainder is fixed up to a global phase, which is aligned away."""
    worst = 0.0
    for start in (0, 3, 9):
        a, b = dense(9, 30 + start, precision), dense(2, 40 + start, precision)
        full = cast(ao.compose(a, b, start), precision)
        q = load(full, precision, engine)
        q.dispose(start, 2)
        assert q.num_qubits == 9
        worst = max(worst, max_err(ao.align_phase(read(q), a), a))
    return worst


def decompose_error(engine, precision):
    """kron of two random states; recombining the two results must give the
    original back elementwise (the phase correction goes to the remainder)."""
    worst = 0.0
    for part, start in ((2, 0), (2, 3), (4, 0), (4, 3)):
        a, b = dense(8, 50 + part + start, precision), dense(part, 60 + part + start, precision)
        full = cast(ao.compose(a, b, start), precision)
        q = load(full, precision, engine)
        dest = sim(part, precision, engine)
        q.decompose(start, dest)
        assert q.num_qubits == 8 and dest.num_qubits == part
        rem, got_part = read(q), read(dest)
        assert abs(np.linalg.norm(rem) - 1) < 1e-5 and abs(np.linalg.norm(got_part) - 1) < 1e-5
        worst = max(worst, max_err(ao.compose(rem, got_part, start), full))
    return worst


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dispose_perm(precision):
    err = dispose_perm_error("hip", precision)
    print(f"dispose_perm: {err / EPS[precision]:.2f} eps")
    assert err <= structural_bound(CPU_DISPOSE_PERM, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dispose(precision):
    err = dispose_error("hip", precision)
    print(f"dispose: {err / EPS[precision]:.2f} eps")
    assert err <= structural_bound(CPU_DISPOSE, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decompose(precision):
    err = decompose_error("hip", precision)
    print(f"decompose: {err / EPS[precision]:.2f} eps")
    assert err <= structural_bound(CPU_DECOMPOSE, precision)


# ---- reductions -------------------------------------------------------------------


@pytest.fixture(scope="module", params=[(n, p) for n in (10, 12) for p in PRECISIONS], ids=str)
def loaded(request):
    """(n, precision, cast state, engine holding it); read-only."""
    n, precision = request.param
    state = cast(ao.random_state(n, np.random.default_rng(100 + n)), precision)
    return n, precision, state, load(state, precision)


def close(got, ref, scale, precision, what):
    err = abs(got - ref)
    print(f"{what}: {err / (EPS[precision] * scale):.2f} eps S")
    assert err <= 16 * EPS[precision] * scale, what


def test_prob(loaded):
    n, precision, state, q = loaded
    for qubit in (0, 5, 6, n - 1):
        close(q.prob(qubit), ao.prob(state, qubit), 1.0, precision, f"prob({qubit})")


def test_prob_mask_and_reg(loaded):
    n, precision, state, q = loaded
    top = 1 << (n - 1)
    for mask, perm in ((0b1001001 | top, 0b1000001), (0b100100 | top, top), (0b11000010, 0)):
        close(q.prob_mask(mask, perm), ao.prob_mask(state, mask, perm), 1.0, precision, "prob_mask")
    for start, length, perm in ((4, 4, 0b1010), (0, 3, 5), (n - 2, 2, 1)):
        close(q.prob_reg(start, length, perm), ao.prob_reg(state, start, length, perm), 1.0, precision, "prob_reg")


def test_prob_parity(loaded):
    n, precision, state, q = loaded
    for mask in (1 << 6, 0b1000101 | 1 << (n - 1), (1 << n) - 1):
        close(q.prob_parity(mask), ao.prob_parity(state, mask), 1.0, precision, "prob_parity")


def test_prob_all_and_bits_all(loaded):
    n, precision, state, q = loaded
    for perm in (0, 77, (1 << n) - 1):
        close(q.prob_all(perm), ao.probs(state)[perm], 1.0, precision, "prob_all")
    bits = [6, 0, n - 1]
    got, ref = np.asarray(q.prob_bits_all(bits)), ao.prob_bits_all(state, bits)
    assert got.shape == ref.shape
    for g, r in zip(got, ref):
        close(g, r, 1.0, precision, "prob_bits_all")


def test_expectation_and_variance_bits(loaded):
    n, precision, state, q = loaded
    for bits in ([6, 0, n - 1], list(range(n))):
        v = ao.bit_values(state.size, bits)
        close(q.expectation_bits_all(bits), ao.expectation(state, v), ao.expectation(state, v), precision, "exp")
        close(q.variance_bits_all(bits), ao.variance(state, v), ao.expectation(state, v * v), precision, "var")


def test_expectation_bits_factorized(loaded):
    n, precision, state, q = loaded
    rng = np.random.default_rng(7 + n)
    bits = [int(b) for b in rng.permutation(n)[:5]]
    perms = [int(p) for p in rng.integers(1, 1000, 5)]
    v = ao.bit_values(state.size, bits, perms, 37)
    close(q.expectation_bits_factorized(bits, perms, 37), ao.expectation(state, v), ao.expectation(state, v), precision, "fact")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [10, 12])
def test_highest_prob_all(n, precision):
    base = ao.random_state(n, np.random.default_rng(200 + n))
    for where in (0, 613, (1 << n) - 1):
        state = base.copy()
        state[where] = 0.5  # the others are ~ 2^-(n/2): at most 0.2 even at 4 sigma
        state = cast(state / np.linalg.norm(state), precision)
        assert load(state, precision).highest_prob_all() == where


def test_sum_sqr_diff(loaded):
    """2 - 2 |<b|a>|: each product term carries <= 3 roundings against
    |a_i| |b_i|, so the inner product is good to 4 eps S, S = sum |a_i| |b_i|;
    the factor 2 doubles it."""
    n, precision, state, q = loaded
    other = cast(ao.random_state(n, np.random.default_rng(300 + n)), precision)
    scale = 2 * float(np.sum(np.abs(state) * np.abs(other)))
    close(q.sum_sqr_diff(load(other, precision)), ao.sum_sqr_diff(state, other), scale, precision, "sum_sqr_diff")


def collapsed_close(q, expected, precision, what):
    err = max_err(read(q), expected)
    print(f"{what}: {err / EPS[precision]:.2f} eps")
    assert err <= 16 * EPS[precision], what


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [10, 12])
def test_collapses(n, precision):
    state = cast(ao.random_state(n, np.random.default_rng(400 + n)), precision)
    mask = 0b1000101 | 1 << (n - 1)
    for result in (False, True):
        q = load(state, precision)
        assert q.force_m_parity(mask, result) == result
        collapsed_close(q, ao.project_parity(state, mask, result), precision, "force_m_parity")
    q = load(state, precision)
    assert q.force_m_reg(5, 3, 0b101) == 0b101
    collapsed_close(q, ao.project_mask(state, 0b111 << 5, 0b101 << 5), precision, "force_m_reg")
    q = load(state, precision)
    reg_mask, result = 0b1001 << 3, 0b1000 << 3
    nrm = 1.0 / np.sqrt(ao.prob_mask(state, reg_mask, result))
    q.apply_m(reg_mask, result, complex(nrm))
    collapsed_close(q, ao.project_mask(state, reg_mask, result), precision, "apply_m")


# ---- 24 qubits: k_reduce's grid-stride loop iterates ----------------------------------

ANGLES = [0.3 + 0.11 * k for k in range(24)]


def product_state_error(engine, n, precision):
    """Largest error, in units of S, of the reductions on the product state
    prod_k ry(ANGLES[k])|0> against their closed forms."""
    q = sim(n, precision, engine)
    for k in range(n):
        q.ry(ANGLES[k], k)
    p = [np.sin(ANGLES[k] / 2) ** 2 for k in range(n)]
    worst = 0.0
    for k in (0, 6, n - 1):
        worst = max(worst, abs(q.prob(k) - p[k]))
    bits = [0, 3, 6, 11, n - 1]
    ref = p[0] * (1 - p[3]) * p[6] * (1 - p[11]) * p[n - 1]
    mask = sum(1 << b for b in bits)
    worst = max(worst, abs(q.prob_mask(mask, (1 << 0) | (1 << 6) | (1 << (n - 1))) - ref))
    odd = (1 - np.prod([1 - 2 * p[b] for b in bits])) / 2
    worst = max(worst, abs(q.prob_parity(mask) - odd))
    every = list(range(n))
    mean = sum(p[k] * 2.0**k for k in every)
    worst = max(worst, abs(q.expectation_bits_all(every) - mean) / mean)
    return worst


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reductions_at_24_qubits(precision):
    """2^24 amplitudes against a reduction grid capped at 32768 blocks of
    256 threads: every thread sums two elements."""
    err = product_state_error("hip", 24, precision)
    print(f"24-qubit product state: {err:.3e} (CPU at 16 qubits: {CPU_PRODUCT[precision]:.3e})")
    assert err <= 4 * CPU_PRODUCT[precision]
