"""Checks shared by test_krylov_eigen_cpu.py and test_krylov_eigen_gpu.py: the
same properties of lanczos_lowest_states on the CPU and the HIP engine,
against eigen_oracle (whose docstring has the definition and every tolerance)
and the dense spectrum. Each check prints its figures before it asserts.
"""
import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po
import adjoint_oracle as ao
import krylov_oracle as ko
import krylov_cases as kc
import eigen_oracle as eo

PRECS = kc.PRECS
EPS = ko.EPS
DTYPE = ko.DTYPE
N = 9

# (nev, dim, max_restarts) at tol = 0 on the 9-qubit chain: Orth over 1 to 64
# vectors on each side of both chunk boundaries, the rotation with k in
# {3, 8, 12, 16, 17, 18, 32, 33, 34, 64} and kp in {1, 2, 4, 6, 8, 13, 16}
TRACKING = ((3, 12, 3), (2, 8, 4), (1, 3, 5), (4, 16, 2), (4, 17, 2), (4, 18, 2), (8, 32, 1), (8, 33, 1),
            (8, 34, 1), (8, 64, 0), (8, 64, 1), (8, 18, 3))
DENSE = ((1, 8), (3, 12), (4, 20), (8, 24))


def chain():
    """-> (terms, S, the dense spectrum) of the 9-qubit chain"""
    terms = kc.chain_terms()
    return terms, ko.sum_abs(terms), ko.dense_eigh(N, terms, "chain")[0]


def call(q, terms, nev, dim, tol=0.0, max_restarts=64, prepare=-1):
    v, r, info = q.lanczos_lowest_states(terms, nev, dim, tol, max_restarts, prepare)
    return np.asarray(v), np.asarray(r), info


def blob(v, r, info):
    """everything a call returns, as bytes"""
    return (v.tobytes(), r.tobytes(), bool(info["converged"]), int(info["restarts"]), int(info["applies"]),
            np.asarray(info["history_values"]).tobytes(), np.asarray(info["history_residuals"]).tobytes())


def expected_launches(dims_per_step, launches, restarts, prepare_k=None, state_in_basis=True):
    """the HIP engine's launch counts of one call, from the basis size j of
    every step: applies * L krylov_apply, the orth launches of the chunk rule,
    one krylov_rotate per restart, and krylov_combine only with prepare >= 0
    (prepare_k: the final basis size; sources beyond the state itself, in
    launches of CAP)"""
    counts = {"krylov_apply": len(dims_per_step) * launches,
              "krylov_orth": sum(eo.orth_launches(j) for j in dims_per_step)}
    if restarts:
        counts["krylov_rotate"] = restarts
    if prepare_k is not None:
        sources = prepare_k - 1 if state_in_basis else prepare_k
        counts["krylov_combine"] = max(1, -(-sources // kc.CAP))
    return counts


def steps_of(nev, dim, restarts):
    """basis sizes of the steps of a run without breakdown"""
    keep = eo.keep_rule(nev, dim)
    js = list(range(1, dim + 1))
    for _ in range(restarts):
        js += list(range(keep + 1, dim + 1))
    return js


# ---- oracle tracking ----------------------------------------------------------------


def guard(run, threshold, label):
    """A cycle ends the call when all wanted residuals are <= threshold, that
    is when the largest one is: that one lies a factor 4 or more from the
    threshold in every cycle, on either side, so that rounding cannot change
    the number of cycles. (A single pair may cross the threshold on its way
    down while another is still far above it; that decides nothing.)"""
    worst = np.nanmax(run["history_residuals"], axis=1)
    ok = (worst >= 4 * threshold) | (worst <= threshold / 4)
    print(f"guard {label}: largest residual / threshold per cycle = {np.round(worst / threshold, 2)}")
    assert ok.all(), (label, worst[~ok], threshold)


def tracking(engine, prec, case):
    nev, dim, rs = case
    terms, s, _ = chain()
    psi = kc.random_psi(N, prec)
    want, d, d_vec, r32, r64 = eo.tracking(psi, terms, nev, dim, rs, prec, "chain")
    guard(want, ko.theta(terms, prec), (case, prec))
    guard(r32, ko.theta(terms, "fp32"), (case, "c64"))
    guard(r64, ko.theta(terms, "fp32"), (case, "c128"))
    q = kc.sim(engine, N, prec)
    q.set_state_vector(psi)
    v, r, info = call(q, terms, nev, dim, 0.0, rs)
    assert kc.state_of(q).tobytes() == psi.tobytes()
    tol = max(8 * d, 16 * EPS[prec] * s)
    hv, hr = np.asarray(info["history_values"]), np.asarray(info["history_residuals"])
    assert info["restarts"] == want["restarts"] and info["applies"] == want["applies"], (info, want["restarts"])
    assert hv.shape == hr.shape == (want["restarts"] + 1, nev)
    assert np.array_equal(np.isnan(hv), np.isnan(want["history_values"]))
    ev = float(np.nanmax(np.abs(hv - want["history_values"])))
    er = float(np.nanmax(np.abs(hr - want["history_residuals"])))
    print(f"tracking {case}/{prec}: cycles {info['restarts'] + 1}, applies {info['applies']}, "
          f"d = {d:.3e}, value err = {ev:.3e}, residual err = {er:.3e}, tol = {tol:.3e}")
    assert ev <= tol and er <= tol, (case, ev, er, tol)
    m = len(want["values"])
    assert len(v) == len(r) == m
    assert v.tobytes() == hv[-1, :m].tobytes() and r.tobytes() == hr[-1, :m].tobytes()
    assert bool(info["converged"]) == want["converged"]
    # the lowest Ritz vector; the same call returns the same bytes
    again = call(q, terms, nev, dim, 0.0, rs, 0)
    assert blob(*again) == blob(v, r, info)
    got = kc.state_of(q).astype(np.complex128)
    vtol = max(8 * d_vec[0], 16 * EPS[prec])
    err = kc.phase_distance(got, want["vectors"][0])
    print(f"tracking {case}/{prec}: vector err = {err:.3e}, tol = {vtol:.3e}")
    assert err <= vtol, (case, err, vtol)


# ---- against the dense spectrum ---------------------------------------------------------


def dense_spectrum(engine, prec, nev, dim, tol=1e-2, max_restarts=32):
    terms, s, lam = chain()
    psi = kc.random_psi(N, prec)
    q = kc.sim(engine, N, prec)
    q.set_state_vector(psi)
    v, r, info = call(q, terms, nev, dim, tol, max_restarts)
    floor = 64 * EPS[prec] * s
    err = np.abs(v - lam[:len(v)])
    print(f"dense ({nev}, {dim}) tol {tol}/{prec}: restarts {info['restarts']}, applies {info['applies']}, "
          f"err = {err}, residuals = {r}, floor = {floor:.3e}")
    assert info["converged"] and len(v) == nev
    if tol > 0:
        assert np.all(r <= tol)
        assert np.all(err <= r + floor), (err, r, floor)
    else:
        assert np.all(err <= floor), (err, floor)
    assert kc.state_of(q).tobytes() == psi.tobytes()


def flagship(engine):
    """dim 64 without a restart in fp32: plain Lanczos returns the ground
    level twice and a spurious value there; this returns four distinct levels"""
    terms, s, lam = chain()
    q = kc.sim(engine, N, "fp32")
    q.set_state_vector(kc.random_psi(N, "fp32"))
    v, r, info = call(q, terms, 4, 64, 0.0, 0)
    floor = 64 * EPS["fp32"] * s
    print(f"flagship: values = {v}, dense = {lam[:4]}, residuals = {r}, floor = {floor:.3e}")
    assert len(v) == 4 and info["restarts"] == 0 and info["applies"] == 64
    assert np.all(np.abs(v - lam[:4]) <= floor)
    assert np.all(np.diff(v) > 0.5)


# ---- prepared vectors ---------------------------------------------------------------------


def prepared_vectors(engine, prec, case=(3, 12, 3)):
    nev, dim, rs = case
    terms, s, _ = chain()
    psi = kc.random_psi(N, prec)
    _, d, _, _, _ = eo.tracking(psi, terms, nev, dim, rs, prec, "chain")
    q = kc.sim(engine, N, prec)
    ys = {}
    for i in sorted({0, 1, nev - 1}):
        q.set_state_vector(psi)
        v, r, info = call(q, terms, nev, dim, 0.0, rs, i)
        y = kc.state_of(q).astype(np.complex128)
        ys[i] = y
        dn = abs(float(np.linalg.norm(y)) - 1.0)
        expect = q.expectation_pauli_sum(terms)
        true_res = float(np.linalg.norm(ko.apply_h(y, terms, np.complex128) - v[i] * y))
        rtol = max(8 * d, 64 * EPS[prec] * s)
        print(f"prepare {i}/{prec}: |norm - 1| = {dn:.3e} (bound {16 * dim * EPS[prec]:.3e}), "
              f"<H> - value = {expect - v[i]:.3e} (bound {64 * EPS[prec] * s:.3e}), "
              f"true residual = {true_res:.6e}, returned = {r[i]:.6e}, tol = {rtol:.3e}")
        assert dn <= 16 * dim * EPS[prec]
        assert abs(expect - v[i]) <= 64 * EPS[prec] * s
        assert abs(true_res - r[i]) <= rtol
    for i in ys:
        for j in ys:
            if i < j:
                ov = abs(np.vdot(ys[i], ys[j]))
                print(f"prepare {i},{j}/{prec}: overlap = {ov:.3e}, bound = {64 * dim * EPS[prec]:.3e}")
                assert ov <= 64 * dim * EPS[prec]


# ---- behaviour ---------------------------------------------------------------------------------


def readonly_and_repeatable(engine, prec):
    terms, _, _ = chain()
    psi = kc.random_psi(N, prec)
    q = kc.sim(engine, N, prec)
    q.set_state_vector(psi)
    first = call(q, terms, 3, 12, 0.0, 3)
    assert kc.state_of(q).tobytes() == psi.tobytes()
    assert blob(*call(q, terms, 3, 12, 0.0, 3)) == blob(*first)
    runs = []
    for _ in range(2):
        q.set_state_vector(psi)
        out = call(q, terms, 3, 12, 0.0, 3, 1)
        runs.append((blob(*out), kc.state_of(q).tobytes()))
    assert runs[0] == runs[1]
    assert runs[0][0] == blob(*first)


def widths(engine, n, prec):
    """n = 1, 2: the run ends by breakdown or spans the space"""
    terms = kc.chain_terms(n)
    s = ko.sum_abs(terms)
    lam = ko.dense_eigh(n, terms, ("eigen widths", n))[0]
    psi = kc.random_psi(n, prec, seed=110 + n)
    q = kc.sim(engine, n, prec)
    q.set_state_vector(psi)
    nev, dim = 2, (4 if n <= 2 else 16)
    v, r, info = call(q, terms, nev, dim)
    floor = 64 * EPS[prec] * s
    print(f"width {n}/{prec}: values = {v}, dense = {lam[:nev]}, residuals = {r}, restarts {info['restarts']}, "
          f"applies {info['applies']}, floor = {floor:.3e}")
    assert 1 <= len(v) <= min(nev, 1 << n)
    assert np.all(np.abs(v - lam[:len(v)]) <= floor)
    if n <= 2:
        assert info["restarts"] == 0 and info["applies"] <= (1 << n)
    assert info["converged"] == (len(v) == nev)
    assert kc.state_of(q).tobytes() == psi.tobytes()


def breakdown(engine, prec):
    n = 9
    zsum = [(0.7, [0], [2]), (-0.4, [3, 8], [2, 2]), (0.25, [1, 4, 6], [2, 2, 2]), (0.1, [], [])]
    tol = 16 * EPS[prec] * ko.sum_abs(zsum)
    q = kc.sim(engine, n, prec)
    q.h(1)  # leave something else in the buffer first
    q.set_permutation(0)
    v, r, info = call(q, zsum, 1, 8)
    assert len(v) == 1 and abs(v[0] - 0.65) <= tol and info["converged"] and info["applies"] == 1
    assert r[0] <= ko.theta(zsum, prec) and info["restarts"] == 0
    v, r, info = call(q, zsum, 2, 8)
    assert len(v) == 1 and abs(v[0] - 0.65) <= tol and not info["converged"]
    hv = np.asarray(info["history_values"])
    assert hv.shape == (1, 2) and np.isnan(hv[0, 1])
    # the pair that was not found cannot be prepared; the state stays
    before = kc.state_of(q).tobytes()
    with pytest.raises(RuntimeError, match="LanczosLowestStates: the run ended with fewer"):
        call(q, zsum, 2, 8, 0.0, 64, 1)
    assert kc.state_of(q).tobytes() == before
    # H = 0.7 Z_0 on |+..+>: two vectors span the orbit
    h = [(0.7, [0], [2])]
    q = kc.sim(engine, n, prec)
    for b in range(n):
        q.h(b)
    v, r, info = call(q, h, 2, 4)
    print(f"plus/{prec}: values = {v}, residuals = {r}")
    assert len(v) == 2 and info["converged"] and info["applies"] == 2
    assert np.abs(v - np.array([-0.7, 0.7])).max() <= 16 * EPS[prec] * 0.7


def any_norm(engine, prec, case=(3, 12, 3)):
    nev, dim, rs = case
    terms, s, _ = chain()
    psi = kc.random_psi(N, prec)
    big = kc.random_psi(N, prec, scale=2.5)
    _, d, _, _, _ = eo.tracking(psi, terms, nev, dim, rs, prec, "chain")
    q = kc.sim(engine, N, prec)
    q.set_state_vector(psi)
    v, r, info = call(q, terms, nev, dim, 0.0, rs)
    q.set_state_vector(big)
    vb, rb, infob = call(q, terms, nev, dim, 0.0, rs)
    tol = 2 * max(8 * d, 16 * EPS[prec] * s)  # each run is within tol of the exact-arithmetic one
    print(f"norm 2.5/{prec}: value dev = {np.abs(v - vb).max():.3e}, residual dev = {np.abs(r - rb).max():.3e}, "
          f"tol = {tol:.3e}")
    assert infob["restarts"] == info["restarts"]
    assert np.abs(v - vb).max() <= tol and np.abs(r - rb).max() <= tol
    assert kc.state_of(q).tobytes() == big.tobytes()


def argument_errors(engine, prec):
    n = 5
    terms = kc.chain_terms(n)
    q = kc.sim(engine, n, prec)
    q.h(0)
    before = kc.state_of(q).tobytes()
    p = "LanczosLowestStates: "
    for nev in (0, qa.KRYLOV_EIG_MAX_NEV + 1):
        with pytest.raises(RuntimeError, match=p + "need 1 <= nev <= %d" % qa.KRYLOV_EIG_MAX_NEV):
            q.lanczos_lowest_states(terms, nev, 16)
    for nev, dim in ((2, 3), (8, 9), (2, qa.KRYLOV_MAX_DIM + 1)):
        with pytest.raises(RuntimeError, match=p + r"need nev \+ 2 <= dim <= %d" % qa.KRYLOV_MAX_DIM):
            q.lanczos_lowest_states(terms, nev, dim)
    for tol in (-1e-3, float("nan")):
        with pytest.raises(RuntimeError, match=p + "tol must not be negative"):
            q.lanczos_lowest_states(terms, 2, 8, tol)
    with pytest.raises(RuntimeError, match=p + "max_restarts must not be negative"):
        q.lanczos_lowest_states(terms, 2, 8, 0.0, -1)
    for prepare in (-2, 2):
        with pytest.raises(RuntimeError, match=p + "need -1 <= prepare < nev"):
            q.lanczos_lowest_states(terms, 2, 8, 0.0, 4, prepare)
    for bad, wanted in (([(1.0, [0], [4])], "bad Pauli code"),
                        ([(1.0, [0, 0], [1, 2])], "qubit repeated in a term"),
                        ([(1.0, [n], [1])], "qubit out of range")):
        with pytest.raises(RuntimeError, match=wanted):
            q.lanczos_lowest_states(bad, 2, 8, 0.0, 4, 0)
    assert kc.state_of(q).tobytes() == before
    q.set_state_vector(np.zeros(1 << n, dtype=DTYPE[prec]))
    with pytest.raises(RuntimeError, match=p + "the state has zero norm"):
        q.lanczos_lowest_states(terms, 2, 8, 0.0, 4, 0)
    assert qa.KRYLOV_EIG_MAX_NEV == 8
    # the defaults: nev 2, dim 16, tol 0, max_restarts 64, prepare -1
    q = kc.sim(engine, n, prec)
    q.h(0)
    dv, dr, dinfo = q.lanczos_lowest_states(terms)
    assert blob(*call(q, terms, 2, 16, 0.0, 64, -1)) == blob(np.asarray(dv), np.asarray(dr), dinfo)


# ---- layers ----------------------------------------------------------------------------------------


def layers_match_engine(engine, layers, prec, n, tol):
    """a wrapping stack returns the bare engine's values; tol is the absolute
    tolerance on amplitudes and on values / S and residuals / S"""
    terms = kc.chain_terms(n)
    s = ko.sum_abs(terms)
    bare = kc.sim(engine, n, prec)
    q = kc.sim(engine, n, prec, layers=layers)
    q.set_state_vector(kc.random_psi(n, prec, seed=900 + n))
    psi = kc.state_of(q)
    bare.set_state_vector(psi)
    v, r, info = call(q, terms, 2, 6, 0.0, 3)
    wv, wr, winfo = call(bare, terms, 2, 6, 0.0, 3)
    assert info["restarts"] == winfo["restarts"] and info["applies"] == winfo["applies"]
    assert np.abs(v - wv).max() <= tol * s and np.abs(r - wr).max() <= tol * s
    assert np.linalg.norm(kc.state_of(q).astype(np.complex128) - psi) <= tol
    v, r, info = call(q, terms, 2, 6, 0.0, 3, 1)
    wv, wr, winfo = call(bare, terms, 2, 6, 0.0, 3, 1)
    assert np.abs(v - wv).max() <= tol * s
    assert kc.phase_distance(kc.state_of(q).astype(np.complex128), kc.state_of(bare).astype(np.complex128)) <= tol
