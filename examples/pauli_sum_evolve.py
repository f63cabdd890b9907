"""Time evolution of a Heisenberg chain through `evolve_pauli_sum` — the whole
Hamiltonian in one call, second-order Trotter steps.

H = J * sum_b (X_b X_{b+1} + Y_b Y_{b+1} + Z_b Z_{b+1})

The engine groups the terms by their X/Y mask, exactly as
`expectation_pauli_sum` does: XX and YY of one bond share an in-place pass
over the state and every ZZ term shares the diagonal pass, so a first-order
step costs n passes and a second-order step 2n - 1 (the turn-around group
merges). `examples/pauli_chain_evolve.py` lowers the same strings by hand
into basis changes, CNOT ladders and RZ, which costs several passes per term.

The energy <H> commutes with the exact evolution, so its drift measures the
product formula's error; it shrinks as the step does.

Run: python examples/pauli_sum_evolve.py [--engine cpu|hip] [--qubits N]
"""

import argparse
import sys

sys.path.insert(0, ".")

import qrack_amd as qa

J = 0.5
# Pauli codes matching the C ABI / reference convention: I=0, X=1, Z=2, Y=3
X, Z, Y = 1, 2, 3


def heisenberg_terms(n, j=J):
    terms = []
    for b in range(n - 1):
        for p in (X, Y, Z):
            terms.append((j, [b, b + 1], [p, p]))
    return terms


def neel_like(n, engine):
    """|0101...> tilted a little, so that the chain has dynamics and <H> is not extremal"""
    q = qa.create_simulator(n, engine=engine, seed=5)
    for i in range(n):
        if i & 1:
            q.x(i)
        q.ry(0.3 + 0.1 * i, i)
    return q


def drift(n, engine, terms, total_time, steps):
    q = neel_like(n, engine)
    e0 = q.expectation_pauli_sum(terms)
    worst = 0.0
    for _ in range(4):
        q.evolve_pauli_sum(terms, total_time / 4, steps=steps // 4, order=2)
        worst = max(worst, abs(q.expectation_pauli_sum(terms) - e0))
    return e0, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", default="hip" if qa.hip_device_count() > 0 else "cpu")
    ap.add_argument("--qubits", type=int, default=12)
    args = ap.parse_args()
    n = args.qubits
    terms = heisenberg_terms(n)
    total_time = 2.0
    print(f"engine            : {args.engine}")
    print(f"qubits, terms     : {n}, {len(terms)}")
    for steps in (8, 32):
        plan = qa.pauli_evolve_plan(terms, n, total_time / 4, steps // 4, 2)
        e0, d = drift(n, args.engine, terms, total_time, steps)
        print(f"steps {steps:3d}         : {4 * len(plan)} passes, <H>(0) = {e0:+.6f}, "
              f"max energy drift {d:.2e}")
        if steps == 8:
            coarse = d
    # a second-order formula: 4x smaller steps, about 16x less drift
    assert d < coarse / 4, (coarse, d)
    assert d < 1e-2
    print("OK")


if __name__ == "__main__":
    main()
