"""Dense float64 oracle for pauli_sum_braket, pauli_sum_apply_into and
adjoint_gradient, independent of the C++. Pauli codes and masks are those of
pauli_oracle; rotations are pauli_evolve_oracle.rotate.

    P|i> = i^ny (-1)^popcount(i&z) |i^x>
    (P psi)[k] = i^ny (-1)^popcount((k^x)&z) psi[k^x]
    <phi|P|psi> = sum_i conj(phi[i^x]) i^ny (-1)^popcount(i&z) psi[i]

The circuit is U = U_N ... U_1 on psi_0, psi_k = U_k ... U_1 psi_0 and
lambda_k = U_{k+1}^+ ... U_N^+ H psi_N. For U_k = exp(-i theta_k P_k):

    E = <psi_N|H|psi_N>        dE/dtheta_k = 2 Im <lambda_k|P_k|psi_k>

Ops are the tuples adjoint_gradient takes: ("rot", qubits, paulis, theta
[, trainable]) and ("gate", qubits, matrix[, controls, anti]).

Bounds (eps_R the unit roundoff of the amplitude type, L = launches(terms),
F the number of factors, a dense k-qubit gate counting 2^k):

  braket    |d re|, |d im| <= TOL sum|c| ||phi|| ||psi||, TOL = 1e-6 / 1e-12:
            products in R, sums in double, as for the Pauli-sum expectation,
            with Cauchy-Schwarz in place of sum 2|psi_i||psi_j| <= 1.
  apply     |got_j - want_j| <= 4 L eps_R a_j,
            a_j = |id||psi_j| + sum_g (sum_{t in g}|c_t|) |psi[j^x_g]|:
            3 eps per complex multiply-add, 1 for the weight's rounding, one
            rounding per accumulation (the form of pauli_evolve_oracle.check).
  gradient  |g_k - want_k| <= (12 (3F + L + 2) eps_R + 2 TOL) sum|c|:
            |dg| <= 2 (||d lam|| ||psi|| + ||lam|| ||d psi||) plus the braket's
            own error, ||lam|| <= sum|c|, a factor's 2-norm rounding is
            4 sqrt(2) eps (from the elementwise 4 eps (|c||a| + |s||b|)), psi
            sees at most 2F factors and lam at most F + L. The energy
            Re <lam|psi> is half such a derivative and takes the same bound.
"""
import numpy as np

import pauli_oracle as po
import pauli_evolve_oracle as peo

EPS = peo.EPS
DTYPE = peo.DTYPE
TOL = {"fp32": 1e-6, "fp64": 1e-12}


def _parity(v):
    par = np.zeros(v.size, dtype=np.int64)
    m = v.copy()
    while m.any():
        par ^= m & 1
        m >>= 1
    return par


def pauli_apply(psi, qubits, paulis):
    """P psi"""
    psi = np.asarray(psi, dtype=np.complex128)
    x, z, ny = po.masks(qubits, paulis)
    src = np.arange(psi.size, dtype=np.int64) ^ x
    return (1j ** (ny % 4)) * (1 - 2 * _parity(src & z)) * psi[src]


def braket(phi, psi, terms):
    """<phi| sum_t c_t P_t |psi>, complex"""
    phi = np.asarray(phi, dtype=np.complex128)
    psi = np.asarray(psi, dtype=np.complex128)
    idx = np.arange(psi.size, dtype=np.int64)
    total = 0j
    for c, qs, ps in terms:
        x, z, ny = po.masks(qs, ps)
        phase = (1j ** (ny % 4)) * (1 - 2 * _parity(idx & z))
        total += c * np.sum(np.conj(phi[idx ^ x]) * phase * psi[idx])
    return complex(total)


def apply_sum(psi, terms):
    """-> (H psi, companion a) with
    a_j = |id||psi_j| + sum_g (sum_{t in g}|c_t|) |psi[j^x_g]|"""
    psi = np.asarray(psi, dtype=np.complex128)
    idx = np.arange(psi.size, dtype=np.int64)
    out = np.zeros_like(psi)
    a = np.zeros(psi.size)
    mag = np.abs(psi)
    for c, qs, ps in terms:
        x = po.masks(qs, ps)[0]
        out += c * pauli_apply(psi, qs, ps)
        a += abs(c) * mag[idx ^ x]
    return out, a


def launches(terms):
    """launches of one pass over H: per distinct X/Y mask of the non-identity
    strings, ceil(distinct strings / PAULI_MAX_TERMS); 1 for identities alone"""
    import qrack_amd as qa

    cap = qa.PAULI_MAX_TERMS or 32
    per_x = {}
    for _, qs, ps in terms:
        x, z, _ = po.masks(qs, ps)
        if x or z:
            per_x.setdefault(x, set()).add(z)
    return sum(-(-len(zs) // cap) for zs in per_x.values()) or 1


def gate_offsets(qubits):
    return [sum(((a >> g) & 1) << q for g, q in enumerate(qubits)) for a in range(1 << len(qubits))]


def apply_gate(psi, qubits, matrix, controls=(), anti=False):
    """dense gate in the mtrx_n convention: bit g of a row or column index is
    the value of qubits[g]; controls all set (all clear with anti)"""
    psi = np.asarray(psi, dtype=np.complex128).copy()
    m = np.asarray(matrix, dtype=np.complex128).reshape(1 << len(qubits), -1)
    idx = np.arange(psi.size, dtype=np.int64)
    cmask = sum(1 << c for c in controls)
    tmask = sum(1 << q for q in qubits)
    base = idx[((idx & cmask) == (0 if anti else cmask)) & ((idx & tmask) == 0)]
    offs = gate_offsets(qubits)
    block = np.stack([psi[base + off] for off in offs])
    out = m @ block
    for row, off in zip(out, offs):
        psi[base + off] = row
    return psi


def unpack(op):
    """-> dict with the defaults filled in"""
    if op[0] == "rot":
        return dict(kind="rot", qubits=list(op[1]), paulis=list(op[2]), theta=float(op[3]),
                    trainable=bool(op[4]) if len(op) > 4 else True)
    assert op[0] == "gate"
    return dict(kind="gate", qubits=list(op[1]), matrix=np.asarray(op[2], dtype=np.complex128),
                controls=list(op[3]) if len(op) > 3 else [], anti=bool(op[4]) if len(op) > 4 else False)


def apply_op(psi, op, inverse=False):
    o = unpack(op)
    if o["kind"] == "rot":
        return peo.rotate(psi, o["qubits"], o["paulis"], -o["theta"] if inverse else o["theta"])[0]
    d = 1 << len(o["qubits"])
    m = o["matrix"].reshape(d, d)
    return apply_gate(psi, o["qubits"], m.conj().T if inverse else m, o["controls"], o["anti"])


def run(psi0, ops):
    psi = np.asarray(psi0, dtype=np.complex128).copy()
    for op in ops:
        psi = apply_op(psi, op)
    return psi


def factors(ops):
    """F: a rotation is one factor, a dense k-qubit gate 2^k"""
    return sum(1 if op[0] == "rot" else 1 << len(op[1]) for op in ops)


def gradient(psi0, ops, terms):
    """-> (E, [dE/dtheta_k for the trainable rotations, in op order]) from the
    explicit forward states and lambda_k"""
    states = [np.asarray(psi0, dtype=np.complex128).copy()]
    for op in ops:
        states.append(apply_op(states[-1], op))
    lam = apply_sum(states[-1], terms)[0]
    energy = float(np.real(np.vdot(lam, states[-1])))
    grad = []
    for k in range(len(ops), 0, -1):
        op = ops[k - 1]
        o = unpack(op)
        if o["kind"] == "rot" and o["trainable"]:
            grad.append(2.0 * float(np.imag(np.vdot(lam, pauli_apply(states[k], o["qubits"], o["paulis"])))))
        lam = apply_op(lam, op, inverse=True)
    return energy, np.array(grad[::-1])


def gradient_bound(ops, terms, prec):
    return (12 * (3 * factors(ops) + launches(terms) + 2) * EPS[prec] + 2 * TOL[prec]) * po.abs_coeffs(terms)


def roundtrip_companion(psi0, ops):
    """|psi_0| pushed through |U_k| of every op, forwards and then backwards:
    the companion vector of the state after the call"""
    a = np.abs(np.asarray(psi0, dtype=np.complex128))
    idx = np.arange(a.size, dtype=np.int64)
    for op in list(ops) + list(ops)[::-1]:
        o = unpack(op)
        if o["kind"] == "rot":
            x = po.masks(o["qubits"], o["paulis"])[0]
            a = abs(np.cos(o["theta"])) * a + abs(np.sin(o["theta"])) * a[idx ^ x]
        else:
            # |M| and |M^+| = |M|^T are applied alike: take the larger
            d = 1 << len(o["qubits"])
            m = np.abs(o["matrix"].reshape(d, d))
            a = apply_gate(a, o["qubits"], np.maximum(m, m.T), o["controls"], o["anti"]).real
    return a


def random_unitary(k, rng):
    """QR of a complex Gaussian"""
    d = 1 << k
    g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    q, r = np.linalg.qr(g)
    return q * (np.diag(r) / np.abs(np.diag(r)))
