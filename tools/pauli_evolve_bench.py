"""Pass times of the Pauli-evolution kernels on the HIP engine next to the
in-place H pass, and one Heisenberg-chain Trotter step through
evolve_pauli_sum against the same step lowered by hand into gates.

    python tools/pauli_evolve_bench.py [--widths 28 30] [--out FILE]

fp32. Every measurement is warmed up once, then timed three times with a host
clock around `reps` calls that end in a device synchronise; the three
per-call times (ms) are reported, one JSON line per width.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import qrack_amd as qa

X, Z, Y = 1, 2, 3


def timed(q, fn, reps):
    fn()
    q.finish()
    best = []
    for _ in range(3):
        q.finish()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        q.finish()
        best.append((time.perf_counter() - t0) / reps * 1e3)
    return best


def heisenberg(n):
    t = []
    for b in range(n - 1):
        t += [(1.0, [b, b + 1], [X, X]), (0.8, [b, b + 1], [Y, Y]), (0.6, [b, b + 1], [Z, Z])]
    return t


def hand_step(q, n, tau):
    """first-order step, every string lowered as examples/pauli_chain_evolve.py does:
    basis changes, CNOT, RZ(2 angle), CNOT, basis changes back"""
    for b in range(n - 1):
        for c, p in ((1.0, X), (0.8, Y), (0.6, Z)):
            for k in (b, b + 1):
                if p == Y:
                    q.is_(k)
                if p != Z:
                    q.h(k)
            q.cnot(b, b + 1)
            q.rz(2 * tau * c, b + 1)
            q.cnot(b, b + 1)
            for k in (b, b + 1):
                if p != Z:
                    q.h(k)
                if p == Y:
                    q.s(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[28, 30])
    ap.add_argument("--out", default=None, help="also write all results to this JSON file")
    args = ap.parse_args()
    assert qa.hip_device_count() > 0, "needs a HIP device"
    out = {}
    for n in args.widths:
        q = qa.create_simulator(n, engine="hip", precision="fp32", seed=1)
        for i in range(0, n, 3):
            q.ry(0.4 + 0.1 * i, i)
        q.finish()
        r = {}
        hi, mid = n - 2, n // 2
        r["h_mid_ms"] = timed(q, lambda: q.h(mid), 20)
        r["h_top_ms"] = timed(q, lambda: q.h(n - 1), 20)
        r["single_xx_mid_ms"] = timed(q, lambda: q.pauli_rotation([mid, mid + 1], [X, X], 0.3), 20)
        r["single_xx_top_ms"] = timed(q, lambda: q.pauli_rotation([hi, hi + 1], [X, X], 0.3), 20)
        r["single_x0_ms"] = timed(q, lambda: q.pauli_rotation([0], [X], 0.3), 20)
        r["single_x0xtop_ms"] = timed(q, lambda: q.pauli_rotation([0, n - 1], [X, Y], 0.3), 20)
        bond = [(1.0, [mid, mid + 1], [X, X]), (0.8, [mid, mid + 1], [Y, Y])]
        r["multi_xx_yy_ms"] = timed(q, lambda: q.evolve_pauli_sum(bond, 0.3), 20)
        mixed = bond + [(0.5, [mid, mid + 1], [X, Y])]
        r["multi_re_im_ms"] = timed(q, lambda: q.evolve_pauli_sum(mixed, 0.3), 20)
        zz = [(0.6, [b, b + 1], [Z, Z]) for b in range(n - 1)]
        r["diag_%d_terms_ms" % len(zz)] = timed(q, lambda: q.evolve_pauli_sum(zz, 0.3), 20)
        r["diag_single_ms"] = timed(q, lambda: q.pauli_rotation([3, 9], [Z, Z], 0.3), 20)
        terms = heisenberg(n)
        r["plan_passes_order1"] = len(qa.pauli_evolve_plan(terms, n, 0.05, 1, 1))
        r["plan_passes_order2"] = len(qa.pauli_evolve_plan(terms, n, 0.05, 1, 2))
        r["step_order1_ms"] = timed(q, lambda: q.evolve_pauli_sum(terms, 0.05, 1, 1), 3)
        r["step_order2_ms"] = timed(q, lambda: q.evolve_pauli_sum(terms, 0.05, 1, 2), 3)
        r["step_hand_lowered_ms"] = timed(q, lambda: hand_step(q, n, 0.05), 2)
        out[n] = r
        print(n, json.dumps(r), flush=True)
        del q
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
