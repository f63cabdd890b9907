"""Dense float64 oracle for Pauli-string expectation values, shared by the
Pauli-sum tests. Pauli codes: 0=I, 1=X, 2=Z, 3=Y; qubit 0 is the low bit.

P|i> = i^ny (-1)^popcount(i&z) |i^x>, so
<psi|P|psi> = sum_i conj(psi[i^x]) i^ny (-1)^popcount(i&z) psi[i].
"""
import numpy as np


def masks(qubits, paulis):
    x = z = ny = 0
    for q, p in zip(qubits, paulis):
        if p in (1, 3):
            x |= 1 << q
        if p in (2, 3):
            z |= 1 << q
        if p == 3:
            ny += 1
    return x, z, ny


def expect(sv, qubits, paulis):
    sv = np.asarray(sv, dtype=np.complex128)
    x, z, ny = masks(qubits, paulis)
    idx = np.arange(sv.size, dtype=np.int64)
    par = np.zeros(sv.size, dtype=np.int64)
    m = idx & z
    while m.any():
        par ^= m & 1
        m >>= 1
    phase = (1j ** (ny % 4)) * (1 - 2 * par)
    return float(np.real(np.sum(np.conj(sv[idx ^ x]) * phase * sv[idx])))


def expect_sum(sv, terms):
    return sum(c * expect(sv, qs, ps) for c, qs, ps in terms)


def random_state(n, rng, dtype):
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (v / np.linalg.norm(v)).astype(dtype)


def random_string(n, rng, min_weight=0):
    """Random subset of qubits in random order with random codes 0..3."""
    k = int(rng.integers(max(1, min_weight), n + 1))
    qs = [int(q) for q in rng.permutation(n)[:k]]
    ps = [int(p) for p in rng.integers(0, 4, size=k)]
    return qs, ps


def random_terms(n, rng, count):
    out = []
    for _ in range(count):
        qs, ps = random_string(n, rng)
        out.append((float(rng.uniform(-1, 1)), qs, ps))
    return out


def abs_coeffs(terms):
    return sum(abs(c) for c, _, _ in terms)
