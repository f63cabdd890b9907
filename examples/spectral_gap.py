"""The gap of a transverse-field Ising chain against the field.

H = - sum_i Z_i Z_(i+1) - g sum_i X_i on an open chain. lanczos_lowest_states
returns the two lowest levels and their residual norms from one start vector;
the gap E_1 - E_0 closes like g^n in the ordered phase (g < 1) and opens
linearly in the disordered one. The start vector is a generic product state: a
vector inside one parity sector (all |0>, say) would only ever find that
sector's levels. Each value is checked against a dense diagonalisation: for a
Hermitian H the residual norm bounds the distance to an eigenvalue.

    python examples/spectral_gap.py [--qubits 10] [--points 6] [--engine hip|cpu]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import qrack_amd as qa  # noqa: E402

PAULI = {1: np.array([[0, 1], [1, 0]], dtype=complex), 2: np.diag([1.0 + 0j, -1.0]),
         3: np.array([[0, -1j], [1j, 0]])}


def ising(n, g):
    terms = [(-1.0, [i, i + 1], [2, 2]) for i in range(n - 1)]
    return terms + [(-g, [i], [1]) for i in range(n)]


def dense(n, terms):
    h = np.zeros((1 << n, 1 << n), dtype=complex)
    for c, qs, ps in terms:
        m = np.eye(1, dtype=complex)
        for q in reversed(range(n)):  # qubit 0 is the lowest index bit
            m = np.kron(m, PAULI[ps[qs.index(q)]] if q in qs else np.eye(2))
        h += c * m
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=10)
    ap.add_argument("--points", type=int, default=6)
    ap.add_argument("--engine", default="hip" if qa.hip_device_count() > 0 else "cpu")
    args = ap.parse_args()
    n = args.qubits
    print(f"{n}-qubit transverse-field Ising chain, engine {args.engine}, fp64, nev 2, dim 24")
    print(f"{'g':>6}{'E0':>16}{'E1':>16}{'gap':>14}{'dense gap':>14}{'residual':>11}{'restarts':>9}{'applies':>8}")
    for g in np.linspace(0.6, 1.6, args.points):
        terms = ising(n, float(g))
        q = qa.create_simulator(n, engine=args.engine, precision="fp64", seed=1)
        for b in range(n):
            q.ry(0.4 + 0.11 * b, b)
            q.rz(0.3 + 0.07 * b, b)
        values, residuals, info = q.lanczos_lowest_states(terms, nev=2, dim=min(24, 1 << n), tol=1e-9)
        lam = np.linalg.eigvalsh(dense(n, terms))
        print(f"{g:>6.2f}{values[0]:>16.10f}{values[1]:>16.10f}{values[1] - values[0]:>14.3e}"
              f"{lam[1] - lam[0]:>14.3e}{max(residuals):>11.1e}{info['restarts']:>9}{info['applies']:>8}")
        assert info["converged"], info
        assert np.all(np.abs(values - lam[:2]) <= residuals + 1e-11 * (n + g * n))


if __name__ == "__main__":
    main()
