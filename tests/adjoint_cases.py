"""Checks shared by test_adjoint_cpu.py and test_adjoint_gpu.py: the same
properties on the CPU and the HIP engine, against adjoint_oracle. Every check
takes the engine's name; tolerances are the oracle's (see its docstring).
Each check prints max err / bound before it asserts.
"""
import itertools

import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po
import pauli_evolve_oracle as peo
import adjoint_oracle as ao

PRECS = ("fp32", "fp64")
TOL = ao.TOL
EPS = ao.EPS
DTYPE = ao.DTYPE
N12 = 12


def sim_with_state(engine, n, prec, seed, scale=1.0, layers=None):
    rng = np.random.default_rng(seed)
    if layers is None:
        q = qa.create_simulator(n, engine=engine, precision=prec, seed=1)
    else:
        q = qa.create_simulator(n, layers=layers, precision=prec, seed=1)
    q.set_state_vector((scale * po.random_state(n, rng, np.complex128)).astype(DTYPE[prec]))
    return q, np.asarray(q.get_state_vector())


def fresh(engine, n, prec):
    return qa.create_simulator(n, engine=engine, precision=prec, seed=1)


def check_braket(bra, phi, q, psi, terms, prec, label=""):
    got = q.pauli_sum_braket(bra, terms)
    want = ao.braket(phi, psi, terms)
    bound = TOL[prec] * po.abs_coeffs(terms) * np.linalg.norm(phi) * np.linalg.norm(psi)
    err = max(abs(got.real - want.real), abs(got.imag - want.imag))
    if bound > 0:
        print(f"braket {label}/{prec}: err / bound = {err / bound:.3f}")
    assert err <= bound, (label, got, want, bound)
    return got


def check_apply(q, psi, dest, terms, prec, label=""):
    q.pauli_sum_apply_into(terms, dest)
    got = np.asarray(dest.get_state_vector()).astype(np.complex128)
    want, a = ao.apply_sum(psi, terms)
    scale = ao.launches(terms) * EPS[prec] * a
    err = np.abs(got - want)
    pos = scale > 0
    ratio = float((err[pos] / scale[pos]).max()) if pos.any() else 0.0
    print(f"apply {label}/{prec}: L = {ao.launches(terms)}, max err / (L eps a) = {ratio:.3f} (bound 4)")
    assert np.all(err <= 4 * scale), (label, ratio)
    return got


def pair(engine, n, prec, seed):
    """two independent random states on two simulators, and a third to write into"""
    q, psi = sim_with_state(engine, n, prec, seed)
    b, phi = sim_with_state(engine, n, prec, seed + 1000)
    d, _ = sim_with_state(engine, n, prec, seed + 2000)
    return q, psi, b, phi, d


# ---- 1. widths -----------------------------------------------------------------


def widths(engine, n, prec):
    q, psi, b, phi, d = pair(engine, n, prec, 300 + n)
    rng = np.random.default_rng(310 + n)
    if n <= 2:
        strings = [(list(range(n)), list(ps)) for ps in itertools.product(range(4), repeat=n)]
    else:
        strings = [po.random_string(n, rng) for _ in range(64)]
    for qs, ps in strings:
        terms = [(float(rng.uniform(0.5, 1.5)), qs, ps)]
        check_braket(b, phi, q, psi, terms, prec, f"n{n} {qs} {ps}")
        check_apply(q, psi, d, terms, prec, f"n{n} {qs} {ps}")
    if n > 2:
        terms = po.random_terms(n, rng, 40)
        check_braket(b, phi, q, psi, terms, prec, f"n{n} sum")
        check_apply(q, psi, d, terms, prec, f"n{n} sum")


# ---- 2. partner logic at n = 12 -------------------------------------------------

_STATE12 = {}


def state12(engine, prec):
    """two random 12-qubit states per (engine, precision), made once, never changed,
    and a scratch destination"""
    key = (engine, prec)
    if key not in _STATE12:
        _STATE12[key] = pair(engine, N12, prec, 1200)
    return _STATE12[key]


def x_masks_12():
    top = 1 << (N12 - 1)
    return [0, 1, top, 1 | top, (1 << N12) - 1] + [1 << b for b in (5, 6, 7, 8)]


def strings_for_mask(x):
    """x crossed with ny mod 4, Z factors below/above the top x bit, Y on the
    top x bit; for x = 0, Z strings on the lane, wave and block edges"""
    if not x:
        return [([b], [2]) for b in (0, 5, 6, 7, 8, N12 - 1)] + [([0, 6, N12 - 1], [2, 2, 2])]
    xbits = [b for b in range(N12) if (x >> b) & 1]
    top = xbits[-1]
    free = [b for b in range(N12) if not (x >> b) & 1]
    below = [b for b in free if b < top][-1:]
    above = [b for b in free if b > top][:1]
    z_sets = [[], below, above, below + above]
    out = []
    for ny in range(min(4, len(xbits)) + 1):
        placements = {tuple(xbits[len(xbits) - ny:])}  # Y on the top x bits
        placements.add(tuple(xbits[:ny]))               # Y on the low x bits, X on top
        for ybits in placements:
            for zs in z_sets:
                qs = xbits + zs
                ps = [3 if b in ybits else 1 for b in xbits] + [2] * len(zs)
                out.append((qs, ps))
    return out


def partner_logic(engine, prec, x):
    q, psi, b, phi, d = state12(engine, prec)
    strings = strings_for_mask(x)
    assert {po.masks(qs, ps)[0] for qs, ps in strings} == {x}
    if x:
        assert len({po.masks(qs, ps)[2] % 4 for qs, ps in strings}) == min(4, bin(x).count("1") + 1)
    for qs, ps in strings:
        check_braket(b, phi, q, psi, [(1.0, qs, ps)], prec, f"x{x:03x} {qs} {ps}")
        check_apply(q, psi, d, [(1.0, qs, ps)], prec, f"x{x:03x} {qs} {ps}")
    rng = np.random.default_rng(x)
    terms = [(float(rng.uniform(-1, 1)), qs, ps) for qs, ps in strings]
    check_braket(b, phi, q, psi, terms, prec, f"x{x:03x} sum")
    check_apply(q, psi, d, terms, prec, f"x{x:03x} sum")


# ---- 3. conjugation and aliasing ---------------------------------------------------


def conjugation_and_aliasing(engine, prec):
    n = 9
    q, psi, b, phi, d = pair(engine, n, prec, 930)
    rng = np.random.default_rng(931)
    terms = po.random_terms(n, rng, 20) + [(0.7, [], [])]
    tol = TOL[prec] * po.abs_coeffs(terms) * np.linalg.norm(phi) * np.linalg.norm(psi)
    ab = check_braket(b, phi, q, psi, terms, prec, "ab")
    ba = check_braket(q, psi, b, phi, terms, prec, "ba")
    # H is Hermitian: <a|H|b> = conj <b|H|a>; each side is within tol of the oracle
    assert abs(ab.real - ba.real) <= 2 * tol and abs(ab.imag + ba.imag) <= 2 * tol
    aa = q.pauli_sum_braket(q, terms)
    assert abs(aa.imag) <= tol
    assert abs(aa.real - q.expectation_pauli_sum(terms)) <= 2 * tol
    # identities alone: the complex inner product
    ident = [(0.75, [], []), (-0.25, [3], [0])]
    got = q.pauli_sum_braket(b, ident)
    want = 0.5 * np.vdot(phi, psi)
    assert abs(got.real - want.real) <= TOL[prec] and abs(got.imag - want.imag) <= TOL[prec]
    check_braket(b, phi, q, psi, ident, prec, "identity")
    # any norms: 3.0 and 0.25 scale the value by 0.75
    q3, psi3 = sim_with_state(engine, n, prec, 930, scale=3.0)
    b4, phi4 = sim_with_state(engine, n, prec, 1930, scale=0.25)
    assert abs(np.linalg.norm(psi3) - 3.0) < 1e-5 and abs(np.linalg.norm(phi4) - 0.25) < 1e-5
    scaled = check_braket(b4, phi4, q3, psi3, terms, prec, "norms")
    assert abs(scaled - 0.75 * ab) <= 4 * tol
    # refusals
    with pytest.raises(Exception):
        q.pauli_sum_apply_into(terms, q)
    other = fresh(engine, n + 1, prec)
    with pytest.raises(Exception):
        q.pauli_sum_braket(other, terms)
    with pytest.raises(Exception):
        q.pauli_sum_apply_into(terms, other)
    with pytest.raises(Exception):
        q.pauli_sum_braket(b, [(1.0, [n], [1])])


# ---- 4. chunking ---------------------------------------------------------------------


def terms_sharing_x(x, count, rng):
    """count distinct strings with the same X/Y mask: z runs over distinct masks,
    which mixes the re and the im set"""
    xbits = [b for b in range(N12) if (x >> b) & 1]
    zs = rng.choice(1 << N12, size=count, replace=False)
    terms = []
    for z in zs:
        qs, ps = [], []
        for b in range(N12):
            code = (1 if b in xbits else 0) | (2 if (int(z) >> b) & 1 else 0)
            if code:
                qs.append(b)
                ps.append(code)
        terms.append((float(rng.uniform(-1, 1)), qs, ps))
    return terms


def chunking(engine, prec):
    q, psi, b, phi, d = state12(engine, prec)
    cap = qa.PAULI_MAX_TERMS or 32
    rng = np.random.default_rng(77)
    x = (1 << 1) | (1 << 4) | (1 << 9)
    terms = terms_sharing_x(x, cap + 3, rng)
    assert {po.masks(qs, ps)[0] for _, qs, ps in terms} == {x}
    assert len({po.masks(qs, ps)[2] & 1 for _, qs, ps in terms}) == 2
    assert ao.launches(terms) == 2
    check_braket(b, phi, q, psi, terms, prec, "chunks")
    got = check_apply(q, psi, d, terms, prec, "chunks")
    # the accumulate launch: against the sum of per-term applies
    per_term = np.zeros_like(got)
    a = np.zeros(got.size)
    for c, qs, ps in terms:
        q.pauli_sum_apply_into([(c, qs, ps)], d)
        per_term += np.asarray(d.get_state_vector()).astype(np.complex128)
        a += ao.apply_sum(psi, [(c, qs, ps)])[1]
    # each side is within 4 L eps a of the exact vector (L = 2 here, 1 per term)
    assert np.all(np.abs(got - per_term) <= 4 * 3 * EPS[prec] * a)


# ---- 5. read-only and write-all ---------------------------------------------------------


def readonly_and_writeall(engine, prec):
    q, psi, b, phi, d = state12(engine, prec)
    rng = np.random.default_rng(79)
    terms = po.random_terms(N12, rng, 30) + [(0.3, [], [])]
    before_q, before_b = psi.tobytes(), phi.tobytes()
    first = q.pauli_sum_braket(b, terms)
    assert np.asarray(q.get_state_vector()).tobytes() == before_q
    assert np.asarray(b.get_state_vector()).tobytes() == before_b
    assert q.pauli_sum_braket(b, terms) == first  # fixed reduction order: bit-identical
    # dest's earlier contents do not leak, whatever they were
    check_apply(q, psi, d, terms, prec, "prefilled")
    one = np.asarray(d.get_state_vector()).tobytes()
    d.set_state_vector(po.random_state(N12, rng, DTYPE[prec]))
    q.pauli_sum_apply_into(terms, d)
    assert np.asarray(d.get_state_vector()).tobytes() == one
    assert np.asarray(q.get_state_vector()).tobytes() == before_q
    # identities alone: dest = c psi, one launch
    q.pauli_sum_apply_into([(0.5, [], [])], d)
    got = np.asarray(d.get_state_vector()).astype(np.complex128)
    assert np.all(np.abs(got - 0.5 * psi) <= 4 * EPS[prec] * 0.5 * np.abs(psi))


def pending_basis_state(engine, prec):
    n, p = 9, 0x0A5
    rng = np.random.default_rng(5)
    terms = po.random_terms(n, rng, 20) + [(0.4, [], [])]
    basis = np.zeros(1 << n, dtype=np.complex128)
    basis[p] = 1.0
    q, psi = sim_with_state(engine, n, prec, 50)
    e = fresh(engine, n, prec)
    e.h(1)  # leave something else in the buffer first
    e.set_permutation(p)
    check_braket(e, basis, q, psi, terms, prec, "basis bra")
    e.set_permutation(p)
    check_braket(q, psi, e, basis, terms, prec, "basis ket")
    e.set_permutation(p)
    d = fresh(engine, n, prec)
    d.set_permutation(3)  # a pending state in dest is dropped, not materialised over the result
    check_apply(e, basis, d, terms, prec, "basis source")
    ops = gradient_circuit(n, np.random.default_rng(6))
    e.set_permutation(p)
    check_gradient(e, basis, ops, terms, prec, "basis psi_0")


# ---- 6. gradient ----------------------------------------------------------------------------


def gradient_circuit(n, rng):
    """24 ops: rotations on masks with bit 0, with the top bit, a diagonal
    string, a Y-heavy string, two untrainable rotations, and a 1-, 2- and
    3-qubit random unitary, one controlled and one anti-controlled"""
    top = n - 1
    mid = n // 2
    th = lambda: float(rng.uniform(-1, 1))
    ops = [
        ("rot", [0], [3], th()),
        ("rot", [top], [1], th()),
        ("rot", [0, top], [1, 3], th()),
        ("rot", [1, mid], [2, 2], th()),                       # diagonal, x = 0
        ("gate", [mid], ao.random_unitary(1, rng), [0], False),  # controlled
        ("rot", list(range(min(n, 4))), [3] * min(n, 4), th()),  # Y-heavy
        ("rot", [mid, 0], [1, 2], th(), False),                # untrainable
        ("rot", [1], [1], th()),
        ("gate", [top, 0], ao.random_unitary(2, rng)),
        ("rot", [top, 1], [2, 1], th()),
        ("rot", [2, 3, top], [3, 3, 1], th()),
        ("rot", [top], [2], th()),                             # diagonal on the top bit
        ("rot", list(range(n)), [1] * n, th()),                # every bit flips
        ("gate", [1, 3, 2], ao.random_unitary(3, rng), [4], True),  # anti-controlled
        ("rot", [0, 1], [3, 3], th()),
        ("rot", [mid], [3], th(), False),                      # untrainable
        ("rot", [0, mid, top], [1, 2, 3], th()),
        ("rot", [3, 0], [1, 1], th()),
        ("rot", [2], [2], th()),
        ("rot", [1, 2, 3, 4], [3, 1, 3, 2], th()),
        ("rot", [top, mid], [3, 1], th()),
        ("rot", [0], [1], th()),
        ("rot", [4, 0], [2, 3], th()),
        ("rot", [mid, 1], [1, 1], th()),
    ]
    assert len(ops) == 24 and n >= 5
    return ops


def run_with_gate_calls(q, ops):
    for op in ops:
        o = ao.unpack(op)
        if o["kind"] == "rot":
            q.pauli_rotation(o["qubits"], o["paulis"], o["theta"])
        else:
            q.mtrx_n(o["qubits"], o["matrix"], controls=o["controls"], anti=o["anti"])


def check_gradient(q, psi0, ops, terms, prec, label=""):
    """energy and every entry against the oracle; the state afterwards against
    psi_0. Returns (E, grad)."""
    e, g = q.adjoint_gradient(ops, terms)
    want_e, want_g = ao.gradient(psi0, ops, terms)
    bound = ao.gradient_bound(ops, terms, prec)
    assert g.shape == want_g.shape
    err = max([abs(e - want_e)] + [abs(x - y) for x, y in zip(g, want_g)])
    print(f"gradient {label}/{prec}: F = {ao.factors(ops)}, L = {ao.launches(terms)}, "
          f"max err / bound = {err / bound:.3f}")
    assert err <= bound, (label, err, bound)
    # psi_0 is back, to rounding: 2F factors
    got = np.asarray(q.get_state_vector()).astype(np.complex128)
    a = ao.roundtrip_companion(psi0, ops)
    scale = 2 * max(ao.factors(ops), 1) * EPS[prec] * a
    back = np.abs(got - np.asarray(psi0, dtype=np.complex128))
    pos = scale > 0
    ratio = float((back[pos] / scale[pos]).max()) if pos.any() else 0.0
    print(f"gradient {label}/{prec}: state back within {ratio:.3f} (2F eps a) (bound 4)")
    assert np.all(back <= 4 * scale), (label, ratio)
    return e, g


def gradient(engine, n, prec):
    rng = np.random.default_rng(600 + n)
    ops = gradient_circuit(n, rng)
    terms = po.random_terms(n, rng, 29) + [(0.6, [], [])]
    q, psi0 = sim_with_state(engine, n, prec, 610 + n)
    e, g = check_gradient(q, psi0, ops, terms, prec, f"n{n}")
    trainable = [k for k, op in enumerate(ops) if op[0] == "rot" and ao.unpack(op)["trainable"]]
    assert len(g) == len(trainable) == 19
    # two fresh simulators: the same bits
    q2, _ = sim_with_state(engine, n, prec, 610 + n)
    e2, g2 = q2.adjoint_gradient(ops, terms)
    assert e2 == e and g2.tobytes() == g.tobytes()
    # independently of numpy: the parameter shift through the existing gate
    # calls, exact since E = A + B cos 2 theta + C sin 2 theta in each angle
    bound = 2 * ao.gradient_bound(ops, terms, prec)
    for slot in (0, len(trainable) // 2, len(trainable) - 1):
        k = trainable[slot]
        shifted = []
        for sign in (+1, -1):
            op = ops[k]
            moved = ops[:k] + [(op[0], op[1], op[2], op[3] + sign * np.pi / 4)] + ops[k + 1:]
            s, _ = sim_with_state(engine, n, prec, 610 + n)
            run_with_gate_calls(s, moved)
            shifted.append(s.expectation_pauli_sum(terms))
        shift = shifted[0] - shifted[1]
        print(f"gradient n{n}/{prec}: entry {slot} vs parameter shift, "
              f"err / bound = {abs(g[slot] - shift) / bound:.3f}")
        assert abs(g[slot] - shift) <= bound, (slot, g[slot], shift)


def gradient_edges(engine, prec):
    n = 5
    rng = np.random.default_rng(66)
    terms = po.random_terms(n, rng, 12) + [(0.5, [], [])]
    q, psi0 = sim_with_state(engine, n, prec, 67)
    # N = 0: the plain energy
    e, g = check_gradient(q, psi0, [], terms, prec, "empty")
    assert g.shape == (0,)
    assert abs(e - q.expectation_pauli_sum(terms)) <= 2 * TOL[prec] * po.abs_coeffs(terms)
    # all untrainable
    ops = [("rot", [0, 4], [1, 3], 0.3, False), ("gate", [2], ao.random_unitary(1, rng))]
    q.set_state_vector(psi0)
    e, g = check_gradient(q, psi0, ops, terms, prec, "untrainable")
    assert g.shape == (0,)
    # one op on one qubit
    q1, one = sim_with_state(engine, 1, prec, 68)
    for code in (1, 2, 3, 0):
        q1.set_state_vector(one)
        _, g = check_gradient(q1, one, [("rot", [0], [code], 0.4)], [(1.0, [0], [2]), (0.5, [0], [1])],
                              prec, f"one qubit code {code}")
        assert g.shape == (1,)
    # bad arguments raise
    for bad in (
        [("spin", [0], [1], 0.1)],
        [("rot", [0], [4], 0.1)],
        [("rot", [n], [1], 0.1)],
        [("rot", [0, 0], [1, 1], 0.1)],
        [("gate", [0, 1], np.eye(2))],
        [("gate", [0], np.eye(2), [0], False)],
        [("rot", [0], [1])],
    ):
        with pytest.raises(Exception):
            q.adjoint_gradient(bad, terms)


# ---- 7. layers ---------------------------------------------------------------------------------


def layers_match_engine(engine, layers, prec, state_tol):
    """a wrapping stack returns the bare engine's values; state_tol is the
    absolute tolerance per unit sum|c|, or None for the oracle's own bounds"""
    n = 9
    rng = np.random.default_rng(700)
    terms = po.random_terms(n, rng, 29) + [(0.6, [], [])]
    ops = gradient_circuit(n, rng)
    bare, psi = sim_with_state(engine, n, prec, 701)
    bare_b, phi = sim_with_state(engine, n, prec, 702)
    q, _ = sim_with_state(engine, n, prec, 701, layers=layers)
    b, _ = sim_with_state(engine, n, prec, 702, layers=layers)
    d, _ = sim_with_state(engine, n, prec, 703, layers=layers)
    c = po.abs_coeffs(terms)
    tol = (state_tol if state_tol is not None else 2 * TOL[prec]) * c
    want = bare.pauli_sum_braket(bare_b, terms)
    assert abs(q.pauli_sum_braket(b, terms) - want) <= 2 * tol
    assert abs(q.pauli_sum_braket(bare_b, terms) - want) <= 2 * tol  # a bare bra under a wrapped ket
    if state_tol is None:
        check_apply(q, psi, d, terms, prec, "-".join(layers))
    else:
        q.pauli_sum_apply_into(terms, d)
        got = np.asarray(d.get_state_vector()).astype(np.complex128)
        assert np.all(np.abs(got - ao.apply_sum(psi, terms)[0]) <= tol)
    with pytest.raises(Exception):
        q.pauli_sum_apply_into(terms, q)
    e, g = q.adjoint_gradient(ops, terms)
    want_e, want_g = bare.adjoint_gradient(ops, terms)
    gtol = state_tol * c if state_tol is not None else ao.gradient_bound(ops, terms, prec)
    assert abs(e - want_e) <= gtol and np.all(np.abs(g - want_g) <= gtol)
    back = np.asarray(q.get_state_vector()).astype(np.complex128)
    if state_tol is None:
        back_tol = 4 * 2 * ao.factors(ops) * EPS[prec] * ao.roundtrip_companion(psi, ops)
    else:
        back_tol = state_tol
    assert np.all(np.abs(back - psi) <= back_tol)
