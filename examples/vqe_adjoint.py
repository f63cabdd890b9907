"""Gradient-descent VQE with adjoint-method gradients: the 6-qubit open
antiferromagnetic Heisenberg chain

    H = sum_i (X_i X_{i+1} + Y_i Y_{i+1} + Z_i Z_{i+1})

`adjoint_gradient` returns the energy and all 33 derivatives from one forward
pass, one application of H and one backward sweep; a parameter-shift gradient
would run the circuit 66 times.

Ansatz: from the Neel state |010101>, three layers of exp(-i theta Y_q) on
every qubit (an RY(2 theta)) and exp(-i theta Z_q Z_{q+1}) on every bond, all
33 angles trainable.

The best product state of this chain is the Neel state with E_NEEL = -5 (one
<ZZ> = -1 per bond, nothing from XX and YY); the exact ground energy E_0, from
numpy.linalg.eigvalsh below, is about -9.974. What lies between the two is
correlation energy that only an entangled state reaches. The run has to
recover more than half of it: it must end below E_0 + GAP with
GAP = (E_NEEL - E_0) / 2. (This shallow ansatz levels off near -8.28, about
two thirds of the way; it is an example of the optimisation loop, not a
recipe for the ground state.)

Run: python examples/vqe_adjoint.py
"""

import sys

sys.path.insert(0, ".")

import numpy as np

import qrack_amd as qa

N = 6
LAYERS = 3
E_NEEL = -(N - 1.0)  # best product state: <ZZ> = -1 on every bond
X, Z, Y = 1, 2, 3

TERMS = [(1.0, [i, i + 1], [p, p]) for i in range(N - 1) for p in (X, Y, Z)]


def exact_ground():
    paulis = {
        X: np.array([[0, 1], [1, 0]], dtype=complex),
        Y: np.array([[0, -1j], [1j, 0]], dtype=complex),
        Z: np.array([[1, 0], [0, -1]], dtype=complex),
    }
    h = np.zeros((1 << N, 1 << N), dtype=complex)
    for c, qs, ps in TERMS:
        m = np.eye(1)
        for q in range(N):  # qubit 0 is the LOW bit: kron(high, low)
            m = np.kron(paulis[ps[qs.index(q)]] if q in qs else np.eye(2), m)
        h += c * m
    return float(np.linalg.eigvalsh(h)[0])


def ansatz(theta):
    ops, k = [], 0
    for _ in range(LAYERS):
        for q in range(N):
            ops.append(("rot", [q], [Y], float(theta[k])))
            k += 1
        for q in range(N - 1):
            ops.append(("rot", [q, q + 1], [Z, Z], float(theta[k])))
            k += 1
    return ops


def main(steps=300, rate=0.03, verbose=True):
    ground = exact_ground()
    gap = 0.5 * (E_NEEL - ground)  # the descent must end below ground + gap
    q = qa.create_simulator(N, engine="cpu", precision="fp64", seed=7)
    rng = np.random.default_rng(11)
    theta = rng.uniform(-0.3, 0.3, size=LAYERS * (2 * N - 1))
    energy = None
    for step in range(steps):
        q.set_permutation(0b010101)
        energy, grad = q.adjoint_gradient(ansatz(theta), TERMS)
        if verbose and step % 50 == 0:
            print(f"step {step:3d}: E = {energy:+.6f}, |grad| = {np.linalg.norm(grad):.3e}")
        theta -= rate * grad
    q.set_permutation(0b010101)
    energy, _ = q.adjoint_gradient(ansatz(theta), TERMS)
    if verbose:
        print(f"exact ground energy : {ground:+.6f}")
        print(f"VQE energy          : {energy:+.6f}  ({len(theta)} parameters, {steps} steps)")
        print(f"required            : below {ground + gap:+.6f} (ground + {gap:.6f})")
    assert energy < ground + gap, (energy, ground, gap)
    if verbose:
        print("OK")
    return energy, ground, gap


if __name__ == "__main__":
    main()
