"""Dense float64 oracle for pauli_rotation and evolve_pauli_sum, shared by the
Pauli-evolution tests. Pauli codes and masks are those of pauli_oracle.

evolve_pauli_sum(terms, time, steps, order) is defined as a product of
per-term rotations exp(-i a P) = cos(a) - i sin(a) P. The order of the
factors comes from the canonical form, rebuilt here from the definition and
independently of the C++: identities summed into one phase, equal (x, z)
merged, strings sorted by x, then by the parity of their Y count (even
first), then by z. A first-order step applies the factors at tau in that
order, a second-order step applies them at tau/2 and then again at tau/2 in
reverse order; the identity phase e^{-i time c} is applied last.

Each factor is applied by index arithmetic:
    (P psi)[k] = i^ny (-1)^popcount((k^x)&z) psi[k^x].
Alongside psi the oracle carries the companion vector of gate_cases.py,
|psi| pushed through |cos| + |sin| P of every factor, and counts the factors
G. The bounds (derived in gate_cases.py: 3 eps per 2x2, plus 1 for entries
formed from an angle):
    |got_i - want_i| <= 4 G eps_R a_i        | ||got||^2 - 1 | <= 8 G eps_R
An engine that serves several factors in one pass rounds less often than the
oracle has factors, so the bound holds for it a fortiori. For the angle's own
rounding to stay inside the "+1", callers keep |tau| sum|coeff| of any one
X/Y mask at or below 1.
"""
import numpy as np

import pauli_oracle as po

EPS = {"fp32": 2.0**-23, "fp64": 2.0**-52}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}


def _parity(v):
    par = np.zeros(v.size, dtype=np.int64)
    m = v.copy()
    while m.any():
        par ^= m & 1
        m >>= 1
    return par


def canonical(terms):
    """-> (summed identity coefficient, [(x, z, coeff)] in application order)"""
    identity = 0.0
    merged = {}
    for c, qs, ps in terms:
        x, z, _ = po.masks(qs, ps)
        if x == 0 and z == 0:
            identity += c
        else:
            merged[(x, z)] = merged.get((x, z), 0.0) + c
    keys = sorted(merged, key=lambda k: (k[0], bin(k[0] & k[1]).count("1") & 1, k[1]))
    return identity, [(x, z, merged[(x, z)]) for x, z in keys]


def factor_list(terms, time, steps=1, order=1):
    """-> (identity phase angle, [(x, z, angle)] over the whole call)"""
    assert order in (1, 2) and steps >= 1
    identity, strings = canonical(terms)
    tau = time / steps
    seq = []
    for _ in range(steps):
        if order == 1:
            seq += [(x, z, tau * c) for x, z, c in strings]
        else:
            half = [(x, z, tau / 2 * c) for x, z, c in strings]
            seq += half + half[::-1]
    return time * identity, seq


def group_load(terms, time, steps=1, order=1):
    """largest |tau| sum|coeff| over the X/Y masks: callers keep it <= 1"""
    _, strings = canonical(terms)
    per_x = {}
    for x, _, c in strings:
        per_x[x] = per_x.get(x, 0.0) + abs(c)
    return abs(time / steps) * max(per_x.values(), default=0.0)


def apply_factor(psi, a, x, z, angle):
    idx = np.arange(psi.size, dtype=np.int64)
    src = idx ^ x
    ny = bin(x & z).count("1")
    p_psi = (1j ** (ny % 4)) * (1 - 2 * _parity(src & z)) * psi[src]
    c, s = np.cos(angle), np.sin(angle)
    return c * psi - 1j * s * p_psi, abs(c) * a + abs(s) * a[src]


def evolve(sv, terms, time, steps=1, order=1):
    """-> (state, companion vector, number of factors G)"""
    psi = np.asarray(sv, dtype=np.complex128).copy()
    a = np.abs(psi)
    phase, seq = factor_list(terms, time, steps, order)
    for x, z, angle in seq:
        psi, a = apply_factor(psi, a, x, z, angle)
    gates = len(seq)
    if phase != 0.0:
        psi = np.exp(-1j * phase) * psi
        gates += 1
    return psi, a, gates


def rotate(sv, qubits, paulis, theta):
    return evolve(sv, [(1.0, qubits, paulis)], theta)


def check(got, want, a, gates, prec, label=""):
    """print the figures, then assert the elementwise and the norm bound"""
    got = np.asarray(got).astype(np.complex128)
    eps = EPS[prec]
    gates = max(gates, 1)
    err = np.abs(got - want)
    scale = gates * eps * a
    pos = scale > 0
    ratio = float((err[pos] / scale[pos]).max()) if pos.any() else 0.0
    norm2 = float(np.vdot(got, got).real)
    print(f"{label}/{prec}: G = {gates}, max err / (G eps a) = {ratio:.3f} (bound 4), "
          f"|norm^2 - 1| / (G eps) = {abs(norm2 - 1) / (gates * eps):.3f} (bound 8)")
    assert np.all(err <= 4 * scale), f"{label}: error {ratio:.3f} G eps a exceeds 4 G eps a"
    assert abs(norm2 - 1.0) <= 8 * gates * eps, f"{label}: norm^2 = {norm2!r}"
