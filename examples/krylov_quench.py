"""Quench of a 10-qubit Heisenberg chain from the Neel state: Krylov evolution
against the second-order product formula, both measured against a dense
reference.

The Krylov call returns an a-posteriori error estimate with the state; the
product formula's error is invisible to its caller. Both runs below apply H
about the same number of times.

    python examples/krylov_quench.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import qrack_amd as qa  # noqa: E402

N = 10
TIME = 1.0
PAULI = {1: np.array([[0, 1], [1, 0]], dtype=complex), 2: np.diag([1.0 + 0j, -1.0]),
         3: np.array([[0, -1j], [1j, 0]])}


def heisenberg(n, field=0.5):
    terms = []
    for i in range(n - 1):
        terms += [(1.0, [i, i + 1], [p, p]) for p in (1, 3, 2)]
    terms += [(field * (-1) ** i, [i], [2]) for i in range(n)]
    return terms


def dense(n, terms):
    h = np.zeros((1 << n, 1 << n), dtype=complex)
    for c, qs, ps in terms:
        m = np.eye(1, dtype=complex)
        for q in reversed(range(n)):  # qubit 0 is the lowest index bit
            m = np.kron(m, PAULI[ps[qs.index(q)]] if q in qs else np.eye(2))
        h += c * m
    return h


def neel(engine, precision):
    q = qa.create_simulator(N, engine=engine, precision=precision, seed=1)
    for i in range(0, N, 2):
        q.x(i)
    return q


def main():
    engine = "hip" if qa.hip_device_count() > 0 else "cpu"
    terms = heisenberg(N)
    lam, vecs = np.linalg.eigh(dense(N, terms))
    psi0 = np.asarray(neel(engine, "fp64").get_state_vector()).astype(complex)
    exact = (vecs * np.exp(-1j * TIME * lam)) @ (vecs.conj().T @ psi0)
    print(f"{N}-qubit Heisenberg chain, Neel state, time {TIME}, engine {engine}, fp64")
    print(f"{'method':<28}{'H applications':>16}{'error':>12}{'estimate':>12}")
    worst = 0.0
    for dim, steps in ((8, 4), (16, 2), (24, 1)):
        q = neel(engine, "fp64")
        est = q.krylov_evolve_pauli_sum(terms, TIME, dim=dim, steps=steps)
        err = float(np.linalg.norm(np.asarray(q.get_state_vector()) - exact))
        print(f"{'krylov dim %d x %d steps' % (dim, steps):<28}{dim * steps:>16}{err:>12.2e}{est:>12.2e}")
        worst = max(worst, err - est)
    for steps in (8, 16, 32):
        q = neel(engine, "fp64")
        q.evolve_pauli_sum(terms, TIME, steps=steps, order=2)
        err = float(np.linalg.norm(np.asarray(q.get_state_vector()) - exact))
        print(f"{'trotter order 2 x %d steps' % steps:<28}{2 * steps:>16}{err:>12.2e}{'-':>12}")
    # the estimate is the caller's handle on the error: it must not be
    # undercut by more than rounding
    assert worst <= 1e-10, worst
    return worst


if __name__ == "__main__":
    main()
