"""Entanglement growth after a quench of a 12-qubit Heisenberg chain.

The chain starts in the Neel product state |0101...> and evolves under
H = sum_i (X_i X_i+1 + Y_i Y_i+1 + Z_i Z_i+1) with evolve_pauli_sum (second
order product formula). After every step the half-chain reduced density
matrix gives the entanglement entropy and the purity: the entropy starts at 0
and grows roughly linearly until it saturates near the half-chain maximum.

    python examples/entanglement_growth.py [--engine cpu|hip|auto]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import qrack_amd as qa


def run(n=12, steps=12, dt=0.1, engine="auto"):
    if engine == "auto":
        engine = "hip" if qa.hip_device_count() > 0 else "cpu"
    q = qa.create_simulator(n, engine=engine, precision="fp64", seed=1)
    q.set_permutation(sum(1 << i for i in range(1, n, 2)))
    terms = [(1.0, [i, i + 1], [p, p]) for i in range(n - 1)
             for p in (qa.Pauli_X, qa.Pauli_Y, qa.Pauli_Z)]
    half = list(range(n // 2))
    print("%d-qubit Heisenberg chain on engine=%s, half chain = qubits %s" % (n, engine, half))
    entropies = []
    for step in range(steps + 1):
        if step:
            q.evolve_pauli_sum(terms, dt, steps=2, order=2)
        s = max(0.0, qa.entanglement_entropy(q, half))
        entropies.append(s)
        print("t=%.2f purity %.6f entropy %.6f" % (step * dt, qa.purity(q, half), s))
    return entropies


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", default="auto", choices=("auto", "cpu", "hip"))
    ap.add_argument("--steps", type=int, default=12)
    args = ap.parse_args()
    run(steps=args.steps, engine=args.engine)
