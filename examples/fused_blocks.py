"""Pre-fused circuit blocks: a brickwork of random SU(4)s on 12 qubits, applied
gate by gate with mtrx_2q and block by block with mtrx_n.

The brickwork alternates layers of gates on pairs (0,1), (2,3), ... and
(1,2), (3,4), ... Every gate is assigned to a 4-qubit window it fits in; a run
of consecutive gates in one window is multiplied into one 16 x 16 in numpy and
applied with a single mtrx_n call, which costs one pass over the state instead
of one per gate. The two final states agree to rounding.

    python examples/fused_blocks.py [--engine cpu|hip|auto] [--layers N]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import qrack_amd as qa


def random_su4(rng):
    z = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    q, r = np.linalg.qr(z)
    u = q * (np.diag(r) / np.abs(np.diag(r)))
    return u / np.linalg.det(u) ** 0.25


def brickwork(n, layers, rng):
    """[(q1, q2, 4x4)], in circuit order; the 4x4 is in mtrx_2q's basis, index
    2 * bit(q2) + bit(q1)."""
    gates = []
    for layer in range(layers):
        for q1 in range(layer % 2, n - 1, 2):
            gates.append((q1, q1 + 1, random_su4(rng)))
    return gates


def embed(u, q1, q2, window):
    """The 4x4 on (q1, q2) as a 16 x 16 on the window's four qubits: bit g of a
    row or column index is the value of window[g]."""
    g1, g2 = window.index(q1), window.index(q2)
    full = np.zeros((16, 16), dtype=np.complex128)
    for col in range(16):
        sub = ((col >> g2) & 1) * 2 + ((col >> g1) & 1)
        rest = col & ~((1 << g1) | (1 << g2))
        for out in range(4):
            row = rest | ((out & 1) << g1) | ((out >> 1) << g2)
            full[row, col] = u[out, sub]
    return full


def fuse(gates, n):
    """[(window, 16 x 16)]: consecutive gates that fit the current window are
    multiplied into its matrix; a gate that does not fit opens a new window."""
    blocks = []
    window, acc = None, None
    for q1, q2, u in gates:
        if window is None or q1 not in window or q2 not in window:
            if window is not None:
                blocks.append((window, acc))
            # the aligned window of four, or one that straddles two of them
            lo = min(q1 - q1 % 4 if q1 % 4 != 3 else q1 - 1, n - 4)
            window, acc = list(range(lo, lo + 4)), np.eye(16, dtype=np.complex128)
        acc = embed(u, q1, q2, window) @ acc
    blocks.append((window, acc))
    return blocks


def run(n=12, layers=8, engine="auto", seed=3):
    if engine == "auto":
        engine = "hip" if qa.hip_device_count() > 0 else "cpu"
    gates = brickwork(n, layers, np.random.default_rng(seed))
    blocks = fuse(gates, n)

    by_gate = qa.create_simulator(n, engine=engine, precision="fp64", seed=1)
    for q1, q2, u in gates:
        by_gate.mtrx_2q([complex(x) for x in u.ravel()], q1, q2)
    by_block = qa.create_simulator(n, engine=engine, precision="fp64", seed=1)
    for window, m in blocks:
        by_block.mtrx_n(window, m)

    a = np.asarray(by_gate.get_state_vector())
    b = np.asarray(by_block.get_state_vector())
    fidelity = float(abs(np.vdot(a, b)) ** 2)
    print("%d qubits, %d layers on engine=%s: %d mtrx_2q calls, %d mtrx_n calls"
          % (n, layers, engine, len(gates), len(blocks)))
    print("fidelity %.12f" % fidelity)
    return fidelity


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", default="auto", choices=("auto", "cpu", "hip"))
    ap.add_argument("--layers", type=int, default=8)
    args = ap.parse_args()
    run(layers=args.layers, engine=args.engine)
