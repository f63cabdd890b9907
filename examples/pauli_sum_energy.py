"""Energy of a Heisenberg chain on a short ansatz through
`expectation_pauli_sum` — the whole Hamiltonian in one call.

H = J * sum_b (X_b X_{b+1} + Y_b Y_{b+1} + Z_b Z_{b+1})

The engine groups the terms by their X/Y mask: XX and YY on one bond share
a read-only pass over the state, and every ZZ term shares the diagonal
pass, so the 3(n-1) terms cost n passes, with no clone and no write to the
state. The result is checked against dense numpy at 8 qubits.

Run: python examples/pauli_sum_energy.py
"""

import sys

sys.path.insert(0, ".")

import numpy as np

import qrack_amd as qa

N = 8
J = 0.5
# Pauli codes matching the C ABI / reference convention: I=0, X=1, Z=2, Y=3
X, Z, Y = 1, 2, 3


def heisenberg_terms(n, j=J):
    terms = []
    for b in range(n - 1):
        for p in (X, Y, Z):
            terms.append((j, [b, b + 1], [p, p]))
    return terms


def ansatz(n, engine):
    q = qa.create_simulator(n, engine=engine, seed=5)
    for i in range(n):
        q.ry(0.3 + 0.17 * i, i)
    for i in range(n - 1):
        q.cnot(i, i + 1)
    for i in range(n):
        q.rz(0.1 * (i + 1), i)
        q.ry(-0.2 + 0.05 * i, i)
    return q


def dense_energy(sv, terms):
    """<psi|H|psi> in float64 with explicit Kronecker products (qubit 0 is the low bit)."""
    mats = {
        0: np.eye(2, dtype=complex),
        X: np.array([[0, 1], [1, 0]], dtype=complex),
        Y: np.array([[0, -1j], [1j, 0]], dtype=complex),
        Z: np.array([[1, 0], [0, -1]], dtype=complex),
    }
    n = int(np.log2(sv.size))
    sv = np.asarray(sv, dtype=np.complex128)
    e = 0.0
    for c, qs, ps in terms:
        ops = dict(zip(qs, ps))
        m = np.array([[1.0 + 0j]])
        for q in range(n - 1, -1, -1):
            m = np.kron(m, mats[ops.get(q, 0)])
        e += c * float(np.real(np.vdot(sv, m @ sv)))
    return e


def main():
    engine = "hip" if qa.hip_device_count() > 0 else "cpu"
    terms = heisenberg_terms(N)
    q = ansatz(N, engine)
    e = q.expectation_pauli_sum(terms)
    e_dense = dense_energy(np.asarray(q.get_state_vector()), terms)
    print(f"engine                : {engine}")
    print(f"terms                 : {len(terms)}")
    print(f"expectation_pauli_sum : {e:+.7f}")
    print(f"dense numpy           : {e_dense:+.7f}")
    print(f"error                 : {abs(e - e_dense):.2e}")
    assert abs(e - e_dense) < 1e-5
    print("OK")


if __name__ == "__main__":
    main()
