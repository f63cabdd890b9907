"""Numpy oracle for lanczos_lowest_states, independent of the C++: a
thick-restart Lanczos with full re-orthogonalisation for the nev lowest
eigenpairs of H, on top of krylov_oracle's apply_h / theta / dense_eigh.

Definition (theta, S, eps_R as in krylov_oracle; CAP = 16):

    threshold = max(tol, theta)
    keep      = min(2 nev, nev + (dim - nev) // 2, dim - 2)

    Orth(w, V = [v_1..v_j]): for round r = 1, 2, for chunks g of CAP
        consecutive vectors in order: c_g = V_g^H w, w <- w - V_g c_g;
        h_i = the sum of c_i over both rounds, complex.

    cycle 0: v_1 = psi / ||psi||
    step j:  w = H v_j; (w, h) = Orth(w, [v_1..v_j]); T[j,j] = Re h_j;
             beta_(j+1) = ||w||; k = j; the cycle stops at k == dim or at
             breakdown beta_(k+1) <= theta; else T[j,j+1] = T[j+1,j] =
             beta_(j+1) and v_(j+1) = w / beta_(j+1).
    end of a cycle: T[:k,:k] = S diag(lambda) S^T, lambda ascending;
             res_i = beta_(k+1) |S[k-1,i]|; the lowest m = min(nev, k) pairs
             join the history. The call ends on breakdown, when all m
             residuals are <= threshold, or when the cycle number equals
             max_restarts. converged = (m == nev and all residuals <= threshold).
    restart: kp = min(keep, k); v~_i = V S[:,i], i < kp; v~_(kp+1) = w / beta_(k+1);
             T~ = diag(lambda_0..lambda_(kp-1)), T~[i,kp] = T~[kp,i] =
             beta_(k+1) S[k-1,i]; go on with step kp + 1.

`dtype` is the type the vectors are held in; scalars, inner products and the
small eigenproblem stay in double.

Tolerances (none taken from the code under test; d is the deviation between
this oracle's complex64 and complex128 runs on the same complex64-rounded
input, scaled by krylov_oracle.scale_to for fp64):

  Ritz values, residuals of every cycle   max(8 d, 16 eps_R S)
  a prepared vector                       max(8 d_vec, 16 eps_R) in phase_distance
  against the dense spectrum              |value_i - lambda_i| <= residual_i + 64 eps_R S
"""
import numpy as np

import krylov_oracle as ko

CAP = 16
EPS = ko.EPS


def keep_rule(nev, dim):
    return min(2 * nev, nev + (dim - nev) // 2, dim - 2)


def orth(w, basis, dtype):
    """two rounds over chunks of CAP; -> (w, h)"""
    h = np.zeros(len(basis), dtype=np.complex128)
    for _ in range(2):
        for g in range(0, len(basis), CAP):
            vg = np.array(basis[g:g + CAP]).astype(np.complex128)
            c = vg.conj() @ w.astype(np.complex128)
            w = (w.astype(np.complex128) - c @ vg).astype(dtype)
            h[g:g + CAP] += c
    return w, h


def lowest_states(psi, terms, nev, dim, tol, max_restarts, prec, dtype=np.complex128):
    """-> dict(values, residuals, converged, restarts, applies, history_values,
    history_residuals (restarts + 1 rows of nev, NaN-padded), vectors (the m
    Ritz vectors of the final cycle, complex128), k (of the final cycle))"""
    psi = np.asarray(psi)
    th = ko.theta(terms, prec)
    threshold = max(tol, th)
    keep = keep_rule(nev, dim)
    norm0 = float(np.linalg.norm(psi.astype(np.complex128)))
    basis = [(psi.astype(np.complex128) / norm0).astype(dtype)]
    t = np.zeros((dim, dim))
    applies = 0
    hist_v, hist_r = [], []
    cycle = 0
    while True:
        broke = False
        j = len(basis) - 1
        while True:
            w = ko.apply_h(basis[j], terms, dtype)
            applies += 1
            w, h = orth(w, basis, dtype)
            t[j, j] = h[j].real
            b = float(np.linalg.norm(w.astype(np.complex128)))
            k = j + 1
            if b <= th:
                broke = True
                break
            if k == dim:
                break
            t[j, j + 1] = t[j + 1, j] = b
            basis.append((w.astype(np.complex128) / b).astype(dtype))
            j += 1
        lam, s = np.linalg.eigh(t[:k, :k])
        res = b * np.abs(s[k - 1, :])
        m = min(nev, k)
        row_v, row_r = np.full(nev, np.nan), np.full(nev, np.nan)
        row_v[:m], row_r[:m] = lam[:m], res[:m]
        hist_v.append(row_v)
        hist_r.append(row_r)
        under = bool(np.all(res[:m] <= threshold))
        if broke or under or cycle == max_restarts:
            vk = np.array(basis[:k]).astype(np.complex128).T
            return {
                "values": lam[:m].copy(), "residuals": res[:m].copy(), "converged": m == nev and under,
                "restarts": cycle, "applies": applies, "history_values": np.array(hist_v),
                "history_residuals": np.array(hist_r), "vectors": [vk @ s[:, i] for i in range(m)], "k": k,
            }
        kp = min(keep, k)
        y = np.array(basis[:k]).astype(np.complex128).T @ s[:, :kp]
        nxt = (w.astype(np.complex128) / b).astype(dtype)
        basis = [y[:, i].astype(dtype) for i in range(kp)] + [nxt]
        t = np.zeros((dim, dim))
        for i in range(kp):
            t[i, i] = lam[i]
            t[i, kp] = t[kp, i] = b * s[k - 1, i]
        cycle += 1


def orth_launches(j):
    """launches of Orth against j vectors on the HIP engine: one chunk is the
    inner products, the update fused with the second round's inner products,
    and the update fused with the norm; more chunks are an inner-product and an
    update launch for every (round, chunk)"""
    chunks = -(-j // CAP)
    return 3 if chunks == 1 else 4 * chunks


_TRACK = {}


def tracking(psi, terms, nev, dim, max_restarts, prec, key):
    """the complex128 oracle on psi and the deviations of the complex64 run:
    -> (want, d for values and residuals, d_vec per Ritz vector, run32, run64)"""
    key = (key, nev, dim, max_restarts, prec)
    if key in _TRACK:
        return _TRACK[key]
    want = lowest_states(psi, terms, nev, dim, 0.0, max_restarts, prec)
    p32 = np.asarray(psi).astype(np.complex64)
    r32 = lowest_states(p32, terms, nev, dim, 0.0, max_restarts, "fp32", np.complex64)
    r64 = lowest_states(p32, terms, nev, dim, 0.0, max_restarts, "fp32")
    assert r32["restarts"] == r64["restarts"], "the two oracle runs take different numbers of cycles"
    d = max(float(np.nanmax(np.abs(r32["history_values"] - r64["history_values"]))),
            float(np.nanmax(np.abs(r32["history_residuals"] - r64["history_residuals"]))))
    d_vec = []
    for a, b in zip(r32["vectors"], r64["vectors"]):
        ov = np.vdot(b, a)
        ph = ov / abs(ov) if abs(ov) > 0 else 1.0
        d_vec.append(float(np.linalg.norm(a - ph * b)) * ko.scale_to(prec))
    _TRACK[key] = (want, d * ko.scale_to(prec), d_vec, r32, r64)
    return _TRACK[key]
