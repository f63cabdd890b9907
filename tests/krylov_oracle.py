"""Numpy oracle for lanczos_tridiagonal, krylov_evolve_pauli_sum and
lanczos_ground_state, independent of the C++.

Definition (c = the canonical sum of `terms`; S = |identity| + sum |w|, the
sum|c| of the other oracles; L = adjoint_oracle.launches(terms); eps_R the unit
roundoff of the amplitude type):

    Lanczos(dim) on psi, ||psi|| > 0:
        v_1 = psi / ||psi||, beta_1 = 0
        for j = 1 .. dim:
            w          = H v_j - beta_j v_(j-1)
            alpha_j    = Re <v_j|w>
            w          = w - alpha_j v_j
            beta_(j+1) = ||w||
            k = j; stop if j == dim or beta_(j+1) <= theta
            v_(j+1)    = w / beta_(j+1)
        theta = 8 (L + 2) eps_R S

H is applied term by term with adjoint_oracle.pauli_apply. `dtype` is the type
the vectors are held in (complex128, or complex64 to emulate an fp32 engine's
rounding); scalars stay in double, and theta always takes the eps of `prec`.
There is no re-orthogonalisation.

Tolerances (none taken from the code under test):

  state     ||got - oracle128|| <= max(8 d, 16 eps_R) ||psi||, d the distance the
            complex64 run shows from the complex128 run on the same case; for
            fp64 d is scaled by eps_64 / eps_32 (rounding error is first-order
            linear in eps). The factor 8 covers another summation order and
            FMA contraction.
  alpha,    |d alpha_j|, |d beta_j| <= max(8 d_T, 16 eps_R S), d_T the largest
  beta      such deviation of the complex64 tridiagonal, scaled the same way.
  estimate  1 % relative, where the oracle's is >= 1e-5 (fp32) / 1e-11 (fp64).
  norm      | ||psi'|| - ||psi|| | <= 16 dim eps_R ||psi||.
"""
import numpy as np

import pauli_oracle as po
import adjoint_oracle as ao

EPS = ao.EPS
DTYPE = ao.DTYPE
EST_FLOOR = {"fp32": 1e-5, "fp64": 1e-11}


def sum_abs(terms):
    """S: coefficients merged per string first, as the canonical sum does"""
    merged = {}
    for c, qs, ps in terms:
        x, z, _ = po.masks(qs, ps)
        merged[(x, z)] = merged.get((x, z), 0.0) + c
    return sum(abs(v) for v in merged.values())


def theta(terms, prec):
    return 8 * (ao.launches(terms) + 2) * EPS[prec] * sum_abs(terms)


def apply_h(v, terms, dtype):
    out = np.zeros(v.size, dtype=np.complex128)
    for c, qs, ps in terms:
        out += c * ao.pauli_apply(v, qs, ps)
    return out.astype(dtype)


def lanczos(psi, terms, dim, prec, dtype=np.complex128):
    """-> (alpha[k], beta[k] = beta_2..beta_(k+1), V = [v_1..v_k], ||psi||)"""
    psi = np.asarray(psi)
    norm0 = float(np.linalg.norm(psi.astype(np.complex128)))
    th = theta(terms, prec)
    v = (psi.astype(np.complex128) / norm0).astype(dtype)
    v_prev = np.zeros_like(v)
    beta_j = 0.0
    alpha, beta, basis = [], [], []
    for j in range(1, dim + 1):
        basis.append(v)
        w = (apply_h(v, terms, dtype).astype(np.complex128) - beta_j * v_prev.astype(np.complex128)).astype(dtype)
        a = float(np.real(np.vdot(v.astype(np.complex128), w.astype(np.complex128))))
        w = (w.astype(np.complex128) - a * v.astype(np.complex128)).astype(dtype)
        b = float(np.linalg.norm(w.astype(np.complex128)))
        alpha.append(a)
        beta.append(b)
        if j == dim or b <= th:
            break
        v_prev, v, beta_j = v, (w.astype(np.complex128) / b).astype(dtype), b
    return np.array(alpha), np.array(beta), basis, norm0


def tridiag(alpha, beta):
    k = len(alpha)
    return np.diag(alpha) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)


def coefficients(alpha, beta, tau):
    """exp(-i tau T_k) e_1 from numpy's eigh"""
    lam, q = np.linalg.eigh(tridiag(np.asarray(alpha, float), np.asarray(beta, float)))
    return (q * np.exp(-1j * tau * lam)) @ q[0, :]


def evolve(psi, terms, time, dim, steps, prec, dtype=np.complex128):
    """-> (state, summed estimate, [k of every step])"""
    psi = np.asarray(psi).astype(dtype)
    if time == 0:
        return psi, 0.0, []
    tau = time / steps
    est, ks = 0.0, []
    for _ in range(steps):
        alpha, beta, basis, norm0 = lanczos(psi, terms, dim, prec, dtype)
        c = coefficients(alpha, beta, tau)
        k = len(alpha)
        est += beta[k - 1] * abs(c[k - 1])
        ks.append(k)
        acc = np.zeros(psi.size, dtype=np.complex128)
        for cj, vj in zip(c, basis):
            acc += cj * vj.astype(np.complex128)
        psi = (norm0 * acc).astype(dtype)
    return psi, float(est), ks


def ground(psi, terms, dim, prec, dtype=np.complex128):
    """-> (lambda, residual, prepared state, k)"""
    alpha, beta, basis, _ = lanczos(psi, terms, dim, prec, dtype)
    lam, q = np.linalg.eigh(tridiag(alpha, beta))
    y = q[:, 0]
    k = len(alpha)
    acc = np.zeros(np.asarray(psi).size, dtype=np.complex128)
    for yj, vj in zip(y, basis):
        acc += yj * vj.astype(np.complex128)
    # "at unit norm": the basis loses orthogonality once a Ritz pair converges
    acc /= np.linalg.norm(acc)
    return float(lam[0]), float(beta[k - 1] * abs(y[k - 1])), acc.astype(dtype), k


def dense_h(n, terms):
    """the 2^n x 2^n matrix of H (n <= 9 in the tests)"""
    dim = 1 << n
    h = np.zeros((dim, dim), dtype=np.complex128)
    eye = np.eye(dim, dtype=np.complex128)
    for c, qs, ps in terms:
        for col in range(dim):
            h[:, col] += c * ao.pauli_apply(eye[:, col], qs, ps)
    return h


_EIGH = {}


def dense_eigh(n, terms, key):
    if key not in _EIGH:
        _EIGH[key] = np.linalg.eigh(dense_h(n, terms))
    return _EIGH[key]


def exact_evolve(psi, n, terms, time, key):
    lam, q = dense_eigh(n, terms, key)
    psi = np.asarray(psi, dtype=np.complex128)
    return (q * np.exp(-1j * time * lam)) @ (q.conj().T @ psi)


def scale_to(prec):
    """what a deviation seen in complex64 is multiplied by for `prec`"""
    return 1.0 if prec == "fp32" else EPS["fp64"] / EPS["fp32"]


def state_tol(psi, terms, time, dim, steps, prec):
    """-> (oracle128 state, oracle estimate, ks, tolerance)"""
    want, est, ks = evolve(psi, terms, time, dim, steps, prec)
    w32, _, _ = evolve(np.asarray(psi).astype(np.complex64), terms, time, dim, steps, "fp32", np.complex64)
    w64, _, _ = evolve(np.asarray(psi).astype(np.complex64), terms, time, dim, steps, "fp32")
    d = float(np.linalg.norm(w32.astype(np.complex128) - w64)) * scale_to(prec)
    norm0 = float(np.linalg.norm(np.asarray(psi).astype(np.complex128)))
    return want, est, ks, max(8 * d, 16 * EPS[prec] * norm0)


def tridiag_tol(psi, terms, dim, prec):
    """-> (alpha, beta of the complex128 oracle, tolerance)"""
    alpha, beta, _, _ = lanczos(psi, terms, dim, prec)
    p32 = np.asarray(psi).astype(np.complex64)
    a32, b32, _, _ = lanczos(p32, terms, dim, "fp32", np.complex64)
    a64, b64, _, _ = lanczos(p32, terms, dim, "fp32")
    m = min(len(a32), len(a64))
    d_t = max(float(np.abs(a32[:m] - a64[:m]).max()), float(np.abs(b32[:m] - b64[:m]).max()))
    return alpha, beta, max(8 * d_t * scale_to(prec), 16 * EPS[prec] * sum_abs(terms))
