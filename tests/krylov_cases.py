"""Checks shared by test_krylov_cpu.py and test_krylov_gpu.py: the same
properties on the CPU and the HIP engine, against krylov_oracle (whose
docstring has the definition and every tolerance). Each check prints its
figures before it asserts.
"""
import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po
import adjoint_oracle as ao
import adjoint_cases as ac
import krylov_oracle as ko

PRECS = ("fp32", "fp64")
EPS = ko.EPS
DTYPE = ko.DTYPE
N12 = ac.N12
CAP = qa.KRYLOV_COMBINE_MAX_VECTORS


def chain_terms(n=9, seed=5):
    """XYZ chain with random X and Z fields and an identity term"""
    rng = np.random.default_rng(seed)
    t = []
    for i in range(n - 1):
        t += [(1.0, [i, i + 1], [1, 1]), (0.8, [i, i + 1], [3, 3]), (0.6, [i, i + 1], [2, 2])]
    for i in range(n):
        t += [(float(rng.uniform(-1, 1)), [i], [1]), (float(rng.uniform(-1, 1)), [i], [2])]
    return t + [(0.3, [], [])]


def sim(engine, n, prec, layers=None):
    if layers is None:
        return qa.create_simulator(n, engine=engine, precision=prec, seed=1)
    return qa.create_simulator(n, layers=layers, precision=prec, seed=1)


_STATES = {}


def random_psi(n, prec, seed=3, scale=1.0):
    """a random state rounded to the engine's type, made once, never changed"""
    key = (n, prec, seed, scale)
    if key not in _STATES:
        v = scale * po.random_state(n, np.random.default_rng(seed), np.complex128)
        _STATES[key] = v.astype(DTYPE[prec])
    return _STATES[key]


def state_of(q):
    return np.asarray(q.get_state_vector())


def combine_launches(k):
    """launches of the combine for k basis vectors: the state and k - 1 sources"""
    return max(1, -(-(k - 1) // CAP))


def check_tridiagonal(q, psi, terms, dim, prec, label=""):
    """alpha, beta against the oracle; the state bit-identical. Returns k."""
    before = state_of(q).tobytes()
    a, b = q.lanczos_tridiagonal(terms, dim)
    wa, wb, tol = ko.tridiag_tol(psi, terms, dim, prec)
    assert len(a) == len(b) == len(wa), (label, len(a), len(wa))
    err = max(float(np.abs(a - wa).max()), float(np.abs(b - wb).max()))
    print(f"tridiagonal {label}/{prec}: k = {len(a)}, err = {err:.3e}, tol = {tol:.3e}")
    assert err <= tol, (label, err, tol)
    assert state_of(q).tobytes() == before
    return len(a)


def check_evolve(q, psi, terms, time, dim, steps, prec, label="", exact=None):
    """state, norm and estimate against the oracle of the same (dim, steps);
    with `exact` also ||got - exact|| <= estimate + tol. Returns (got, est, ks)."""
    est = q.krylov_evolve_pauli_sum(terms, time, dim, steps)
    got = state_of(q).astype(np.complex128)
    want, west, ks, tol = ko.state_tol(psi, terms, time, dim, steps, prec)
    err = float(np.linalg.norm(got - want))
    norm0 = float(np.linalg.norm(np.asarray(psi).astype(np.complex128)))
    print(f"evolve {label}/{prec}: dim {dim} steps {steps} k {ks}, err = {err:.3e}, tol = {tol:.3e}, "
          f"estimate = {est:.6e} (oracle {west:.6e})")
    assert err <= tol, (label, err, tol)
    dn = abs(float(np.linalg.norm(got)) - norm0)
    print(f"evolve {label}/{prec}: norm drift = {dn:.3e}, bound = {16 * dim * EPS[prec] * norm0:.3e}")
    assert dn <= 16 * dim * EPS[prec] * norm0
    if west >= ko.EST_FLOOR[prec]:
        assert abs(est - west) <= 0.01 * west, (label, est, west)
    if exact is not None:
        ex = float(np.linalg.norm(got - exact))
        print(f"evolve {label}/{prec}: ||got - exact|| = {ex:.3e}, estimate + tol = {est * norm0 + tol:.3e}")
        assert ex <= est * norm0 + tol, (label, ex, est, tol)
    return got, est, ks


def both(q, psi, terms, time, dim, prec, label, steps=1):
    """the tridiagonal and the evolved state from psi; returns (k, got)"""
    q.set_state_vector(psi)
    k = check_tridiagonal(q, psi, terms, dim, prec, label)
    got, _, ks = check_evolve(q, psi, terms, time, dim, steps, prec, label)
    if steps == 1:
        assert ks == [k]
    return k, got


# ---- 1. widths ---------------------------------------------------------------------


def widths(engine, n, prec):
    rng = np.random.default_rng(100 + n)
    terms = po.random_terms(n, rng, 12) + [(0.4, [], [])]
    psi = random_psi(n, prec, seed=110 + n)
    q = sim(engine, n, prec)
    time = 0.5 / ko.sum_abs(terms)
    k, got = both(q, psi, terms, time, 4, prec, f"n{n}")
    assert k <= min(4, 1 << n)
    if n <= 2:
        # the space is no larger than dim: the run ends by breakdown or spans
        # it all, and the evolution is exact
        tol = ko.state_tol(psi, terms, time, 4, 1, prec)[3]
        ex = ko.exact_evolve(psi, n, terms, time, ("widths", n))
        assert np.linalg.norm(got - ex) <= tol


# ---- 2. partner logic at 12 qubits ---------------------------------------------------


def mask_group(x):
    """three strings of one X/Y mask: real and (for x != 0) imaginary weights"""
    strings = ac.strings_for_mask(x)
    parity = lambda s: po.masks(*s)[2] & 1
    even = [s for s in strings if not parity(s)]
    odd = [s for s in strings if parity(s)]
    pick = (even[:2] + odd[:1]) if odd else even[:3]
    assert len(pick) == 3 and {po.masks(*s)[0] for s in pick} == {x}
    coeffs = (0.9, -0.6, 0.7)
    return [(c, qs, ps) for c, (qs, ps) in zip(coeffs, pick)]


def partner_logic(engine, prec, x):
    psi = random_psi(N12, prec, seed=1200)
    q = sim(engine, N12, prec)
    group = mask_group(x) + [(0.35, [], [])]
    if x:
        assert any(po.masks(qs, ps)[2] & 1 for _, qs, ps in group[:3])
    both(q, psi, group, 0.2, 3, prec, f"x{x:03x} alone")
    # the same group second: an x = 0 group sorts before it; the x = 0 group
    # itself is followed by another mask, and its accumulating form is the
    # second chunk of chunking()
    other = [(0.5, [3], [2])] if x else [(0.5, [2, 9], [1, 3])]
    terms = group + other
    assert ao.launches(terms) == 2
    both(q, psi, terms, 0.2, 3, prec, f"x{x:03x} second")


# ---- 3. a group larger than the launch table -----------------------------------------


def chunking(engine, prec):
    cap = qa.PAULI_MAX_TERMS or 32
    psi = random_psi(N12, prec, seed=1200)
    q = sim(engine, N12, prec)
    rng = np.random.default_rng(77)
    x = (1 << 1) | (1 << 4) | (1 << 9)
    flip = ac.terms_sharing_x(x, cap + 3, rng)
    diag = [t for t in ac.terms_sharing_x(0, cap + 4, rng) if t[1]][:cap + 3]
    assert ao.launches(flip) == 2 and ao.launches(diag) == 2
    both(q, psi, flip, 0.05, 3, prec, "flip chunks")
    both(q, psi, diag, 0.05, 3, prec, "diagonal chunks")
    both(q, psi, diag + flip + [(0.2, [], [])], 0.05, 3, prec, "both")


# ---- 4. dims ----------------------------------------------------------------------------

DIMS = (1, 2, CAP, CAP + 1, CAP + 2, 2 * CAP, 2 * CAP + 1, 2 * CAP + 2, 64)


def dims(engine, prec, dim):
    """The evolved state at every dim: it is well conditioned, the late
    vectors enter with coefficients that decay faster than exponentially. The
    tridiagonal is compared up to dim CAP + 2 only. Without
    re-orthogonalisation alpha_j and beta_j of a longer run amplify rounding
    exponentially once the extreme Ritz values have converged (from about 25
    steps on in complex64 on this chain), so the first-order scaling of
    krylov_oracle's tolerance says nothing about them. Of a longer run the
    leading CAP + 2 entries are compared, against the oracle of that dim:
    they do not depend on how far the run goes on, and they pin the long
    rotation of the three buffers."""
    n = 9
    terms = chain_terms()
    psi = random_psi(n, prec)
    q = sim(engine, n, prec)
    if dim <= CAP + 2:
        k, got = both(q, psi, terms, 0.3, dim, prec, f"dim{dim}")
    else:
        q.set_state_vector(psi)
        a, b = q.lanczos_tridiagonal(terms, dim)
        k = len(a)
        lead = CAP + 2
        wa, wb, tol = ko.tridiag_tol(psi, terms, lead, prec)
        err = max(float(np.abs(a[:lead] - wa).max()), float(np.abs(b[:lead] - wb).max()))
        print(f"tridiagonal dim{dim}/{prec}: leading {lead} entries, err = {err:.3e}, tol = {tol:.3e}")
        assert len(b) == k and err <= tol
        assert state_of(q).tobytes() == psi.tobytes()
        got, _, ks = check_evolve(q, psi, terms, 0.3, dim, 1, prec, f"dim{dim}")
        assert ks == [k]
    assert k == dim
    if dim == 1:
        # one vector: the phase e^(-i tau alpha_1)
        q.set_state_vector(psi)
        a, _ = q.lanczos_tridiagonal(terms, 1)
        tol = ko.state_tol(psi, terms, 0.3, 1, 1, prec)[3]
        assert np.linalg.norm(got - np.exp(-0.3j * a[0]) * psi.astype(np.complex128)) <= tol


def estimate_cases(engine, prec):
    """(dim, time) = (4, 0.05) and (8, 0.1): the estimate against the oracle's,
    and the true error under it"""
    n = 9
    terms = chain_terms()
    psi = random_psi(n, prec)
    q = sim(engine, n, prec)
    for dim, time in ((4, 0.05), (8, 0.1)):
        q.set_state_vector(psi)
        exact = ko.exact_evolve(psi, n, terms, time, "chain")
        _, est, _ = check_evolve(q, psi, terms, time, dim, 1, prec, f"estimate dim{dim}", exact=exact)
        assert est >= ko.EST_FLOOR[prec]


# ---- 5. breakdown -------------------------------------------------------------------------


def breakdown(engine, prec):
    n = 9
    # a basis state is an eigenvector of a Z-only sum: k = 1, left pending
    zsum = [(0.7, [0], [2]), (-0.4, [3, 8], [2, 2]), (0.25, [1, 4, 6], [2, 2, 2]), (0.1, [], [])]
    q = sim(engine, n, prec)
    q.h(1)  # leave something else in the buffer first
    q.set_permutation(0)
    basis = np.zeros(1 << n, dtype=DTYPE[prec])
    basis[0] = 1.0
    a, b = q.lanczos_tridiagonal(zsum, 8)
    assert len(a) == 1 and abs(a[0] - 0.65) <= 16 * EPS[prec] * ko.sum_abs(zsum) and b[0] <= ko.theta(zsum, prec)
    q.set_permutation(0)
    got, est, ks = check_evolve(q, basis, zsum, 0.9, 8, 1, prec, "basis state")
    assert ks == [1] and est <= ko.theta(zsum, prec)
    # H = 0.7 Z_0 on |+..+>: two vectors span the orbit, exact for any dim >= 2
    h = [(0.7, [0], [2])]
    for dim in (2, 5):
        q = sim(engine, n, prec)
        for b_ in range(n):
            q.h(b_)
        plus = state_of(q)
        a, b = q.lanczos_tridiagonal(h, dim)
        assert len(a) == 2
        got, est, ks = check_evolve(q, plus, h, 3.0, dim, 1, prec, f"plus dim{dim}")
        p = plus.astype(np.complex128)
        exact = np.cos(2.1) * p - 1j * np.sin(2.1) * ao.pauli_apply(p, [0], [2])
        tol = ko.state_tol(plus, h, 3.0, dim, 1, prec)[3]
        assert ks == [2] and np.linalg.norm(got - exact) <= tol


# ---- 6. stepping and edge inputs ---------------------------------------------------------


def stepping_and_edges(engine, prec):
    n = 9
    terms = chain_terms()
    psi = random_psi(n, prec)
    q = sim(engine, n, prec)
    q.set_state_vector(psi)
    check_evolve(q, psi, terms, 0.3, 6, 3, prec, "steps 3")
    # negative time undoes positive time: each call is within tol of its
    # oracle and within its estimate of the exact unitary
    q.set_state_vector(psi)
    est_f = q.krylov_evolve_pauli_sum(terms, 0.1, 16)
    mid = state_of(q)
    tol_f = ko.state_tol(psi, terms, 0.1, 16, 1, prec)[3]
    _, est_b, _ = check_evolve(q, mid, terms, -0.1, 16, 1, prec, "negative time")
    tol_b = ko.state_tol(mid, terms, -0.1, 16, 1, prec)[3]
    back = float(np.linalg.norm(state_of(q).astype(np.complex128) - psi.astype(np.complex128)))
    print(f"undo/{prec}: {back:.3e} <= {tol_f + tol_b + est_f + est_b:.3e}")
    assert back <= tol_f + tol_b + est_f + est_b
    # time 0: nothing happens
    q.set_state_vector(psi)
    assert q.krylov_evolve_pauli_sum(terms, 0.0, 8, 2) == 0.0
    assert state_of(q).tobytes() == psi.tobytes()
    # any norm, which the result keeps
    big = random_psi(n, prec, scale=2.5)
    assert abs(np.linalg.norm(big.astype(np.complex128)) - 2.5) < 1e-5
    q.set_state_vector(big)
    k = check_tridiagonal(q, big, terms, 8, prec, "norm 2.5")
    check_evolve(q, big, terms, 0.1, 8, 1, prec, "norm 2.5")


# ---- 7. read-only calls, repeatability ------------------------------------------------------


def readonly_and_repeatable(engine, prec):
    n = 9
    terms = chain_terms()
    psi = random_psi(n, prec)
    q = sim(engine, n, prec)
    q.set_state_vector(psi)
    a1, b1 = q.lanczos_tridiagonal(terms, 12)
    g1 = q.lanczos_ground_state(terms, 12, False)
    assert state_of(q).tobytes() == psi.tobytes()
    a2, b2 = q.lanczos_tridiagonal(terms, 12)
    assert a1.tobytes() == a2.tobytes() and b1.tobytes() == b2.tobytes()
    assert q.lanczos_ground_state(terms, 12, False) == g1
    runs = []
    for _ in range(2):
        q.set_state_vector(psi)
        est = q.krylov_evolve_pauli_sum(terms, 0.2, 12, 2)
        runs.append((est, state_of(q).tobytes()))
    assert runs[0] == runs[1]
    runs = []
    for _ in range(2):
        q.set_state_vector(psi)
        runs.append((q.lanczos_ground_state(terms, 12, True), state_of(q).tobytes()))
    assert runs[0] == runs[1]
    # prepare=False returns what prepare=True returns
    assert runs[0][0] == g1


# ---- 8. argument errors ------------------------------------------------------------------------


def argument_errors(engine, prec):
    n = 5
    terms = chain_terms(n)
    q = sim(engine, n, prec)
    q.h(0)
    before = state_of(q).tobytes()
    # every refusal is the library's own, by its text
    for dim in (0, qa.KRYLOV_MAX_DIM + 1):
        wanted = "need 1 <= dim <= %d" % qa.KRYLOV_MAX_DIM
        with pytest.raises(RuntimeError, match="LanczosTridiagonal: " + wanted):
            q.lanczos_tridiagonal(terms, dim)
        with pytest.raises(RuntimeError, match="KrylovEvolvePauliSum: " + wanted):
            q.krylov_evolve_pauli_sum(terms, 0.1, dim)
        with pytest.raises(RuntimeError, match="LanczosGroundState: " + wanted):
            q.lanczos_ground_state(terms, dim)
    with pytest.raises(RuntimeError, match="steps must be at least 1"):
        q.krylov_evolve_pauli_sum(terms, 0.1, 4, 0)
    for bad, wanted in (([(1.0, [0], [4])], "bad Pauli code"),
                        ([(1.0, [0, 0], [1, 2])], "qubit repeated in a term"),
                        ([(1.0, [n], [1])], "qubit out of range")):
        with pytest.raises(RuntimeError, match=wanted):
            q.lanczos_tridiagonal(bad, 4)
        with pytest.raises(RuntimeError, match=wanted):
            q.krylov_evolve_pauli_sum(bad, 0.1, 4)
        with pytest.raises(RuntimeError, match=wanted):
            q.lanczos_ground_state(bad, 4, True)
    assert state_of(q).tobytes() == before
    q.set_state_vector(np.zeros(1 << n, dtype=DTYPE[prec]))
    with pytest.raises(RuntimeError, match="zero norm"):
        q.lanczos_tridiagonal(terms, 4)
    with pytest.raises(RuntimeError, match="zero norm"):
        q.krylov_evolve_pauli_sum(terms, 0.1, 4)
    with pytest.raises(RuntimeError, match="zero norm"):
        q.lanczos_ground_state(terms, 4, True)
    assert qa.KRYLOV_MAX_DIM == 64


# ---- ground state ---------------------------------------------------------------------------------


def phase_distance(got, want):
    """2-norm distance up to a global phase"""
    ov = np.vdot(want, got)
    ph = ov / abs(ov) if abs(ov) > 0 else 1.0
    return float(np.linalg.norm(got - ph * want))


def ground_state(engine, prec):
    """three restarts of a 24-vector Lanczos on the 9-qubit chain"""
    n, dim = 9, 24
    terms = chain_terms()
    s = ko.sum_abs(terms)
    lam = ko.dense_eigh(n, terms, "chain")[0]
    floor = 64 * EPS[prec] * s
    psi = random_psi(n, prec)
    q = sim(engine, n, prec)
    q.set_state_vector(psi)
    energy = None
    for call in range(3):
        energy, res = q.lanczos_ground_state(terms, dim, True)
        got = state_of(q).astype(np.complex128)
        near = float(np.abs(lam - energy).min())
        expect = q.expectation_pauli_sum(terms)
        print(f"ground {call}/{prec}: E = {energy:.12f} (lambda_min {lam[0]:.12f}), residual = {res:.3e}, "
              f"nearest eigenvalue at {near:.3e}, <H> - E = {expect - energy:.3e}, floor = {floor:.3e}")
        assert near <= max(res, floor)
        assert energy >= lam[0] - floor
        assert abs(expect - energy) <= floor
        assert abs(np.linalg.norm(got) - 1.0) <= 16 * dim * EPS[prec]
        if call:
            # a restart begins at a nearly converged vector: beta_2 is of the
            # residual's size, v_2 = w / beta_2 magnifies w's rounding by its
            # inverse and the later vectors are made of it. The energies above
            # are what a restart is for; the state is compared where the basis
            # is well conditioned, on the first call
            continue
        # the prepared state against the oracle's, up to a global phase
        want = ko.ground(psi, terms, dim, prec)[2]
        p32 = np.asarray(psi).astype(np.complex64)
        w32 = ko.ground(p32, terms, dim, "fp32", np.complex64)[2].astype(np.complex128)
        w64 = ko.ground(p32, terms, dim, "fp32")[2]
        tol = max(8 * phase_distance(w32, w64) * ko.scale_to(prec), 16 * EPS[prec])
        err = phase_distance(got, want)
        print(f"ground {call}/{prec}: state err = {err:.3e}, tol = {tol:.3e}")
        assert err <= tol
    assert abs(energy - lam[0]) <= floor


# ---- 9. layers ---------------------------------------------------------------------------------------


def layers_match_engine(engine, layers, prec, n, state_tol):
    """a wrapping stack returns the bare engine's values; state_tol is the
    absolute tolerance on amplitudes, alpha / S and beta / S"""
    terms = chain_terms(n)
    s = ko.sum_abs(terms)
    bare = sim(engine, n, prec)
    q = sim(engine, n, prec, layers=layers)
    q.set_state_vector(random_psi(n, prec, seed=900 + n))
    psi = state_of(q)  # what the stack holds (a lossy layer rounds on the way in)
    bare.set_state_vector(psi)
    a, b = q.lanczos_tridiagonal(terms, 6)
    wa, wb = bare.lanczos_tridiagonal(terms, 6)
    assert len(a) == len(wa)
    assert np.abs(a - wa).max() <= state_tol * s and np.abs(b - wb).max() <= state_tol * s
    e, r = q.lanczos_ground_state(terms, 6, False)
    we, wr = bare.lanczos_ground_state(terms, 6, False)
    assert abs(e - we) <= state_tol * s and abs(r - wr) <= state_tol * s
    assert np.linalg.norm(state_of(q).astype(np.complex128) - psi) <= state_tol
    est = q.krylov_evolve_pauli_sum(terms, 0.2, 6, 2)
    west = bare.krylov_evolve_pauli_sum(terms, 0.2, 6, 2)
    assert abs(est - west) <= state_tol * s
    assert np.linalg.norm(state_of(q).astype(np.complex128) - state_of(bare)) <= state_tol
    q.set_state_vector(psi)
    bare.set_state_vector(psi)
    e, r = q.lanczos_ground_state(terms, 6, True)
    we, wr = bare.lanczos_ground_state(terms, 6, True)
    assert abs(e - we) <= state_tol * s
    assert phase_distance(state_of(q).astype(np.complex128), state_of(bare).astype(np.complex128)) <= state_tol
