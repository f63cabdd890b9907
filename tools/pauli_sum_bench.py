"""Heisenberg-chain energy on the HIP engine: per-term pauli_expectation
calls against one expectation_pauli_sum call.

    python tools/pauli_sum_bench.py --mode per-term   # needs nothing new
    python tools/pauli_sum_bench.py --mode sum
    python tools/pauli_sum_bench.py --mode both       # alternates the two per repetition
    python tools/pauli_sum_bench.py --mode yardstick  # read bandwidth and the ALU crossover

Every timed repetition ends in a host synchronisation (each call returns a
value), follows --warmup untimed repetitions, and the median of --reps
repetitions is reported, one JSON line per measurement. Bytes/s is computed
from 2^n * sizeof(amplitude), the bytes one read of the state needs.
"""
import argparse
import json
import os
import statistics
import sys
import time

# an installed or PYTHONPATH-selected qrack_amd wins; the tree is the fallback
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import qrack_amd as qa  # noqa: E402

X, Z, Y = 1, 2, 3


def heisenberg_terms(n, j=0.5):
    return [(j, [b, b + 1], [p, p]) for b in range(n - 1) for p in (X, Y, Z)]


def prepare(n):
    q = qa.create_simulator(n, engine="hip", precision="fp32", seed=5)
    for i in range(n):
        q.ry(0.3 + 0.17 * i, i)
    for i in range(n - 1):
        q.cnot(i, i + 1)
    for i in range(n):
        q.rz(0.1 * (i + 1), i)
    q.prob(0)  # host sync: preparation is outside every timed window
    return q


def per_term(q, terms):
    return sum(c * q.pauli_expectation(qs, ps) for c, qs, ps in terms)


def pauli_sum(q, terms):
    return q.expectation_pauli_sum(terms)


def timed(fn):
    t0 = time.perf_counter()
    v = fn()
    return time.perf_counter() - t0, v


def measure(fns, warmup, reps):
    """fns: {name: callable}; the callables alternate inside every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    value = {}
    for _ in range(reps):
        for k, fn in fns.items():
            dt, value[k] = timed(fn)
            times[k].append(dt)
    return {k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v),
                "value": value[k]} for k, v in times.items()}


def report(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("per-term", "sum", "both", "yardstick"), default="both")
    ap.add_argument("--widths", default="28,30")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")
    if qa.hip_device_count() == 0:
        sys.exit("pauli_sum_bench: no HIP device")

    for n in (int(w) for w in args.widths.split(",")):
        q = prepare(n)
        terms = heisenberg_terms(n)
        state_bytes = (1 << n) * 8
        if args.mode == "yardstick":
            top = n - 1
            group1 = [(1.0, [0, top], [X, X])]
            # 32 strings on one X/Y mask: Z factors on the qubits in between
            group32 = [(1.0, [0, top] + [1 + (k % 5), 8 + (k // 5)], [X, X, Z, Z])
                       for k in range(32)]
            fns = {
                "prob_parity": lambda: q.prob_parity(0b11),
                "single_string": lambda: q.pauli_expectation([0, top], [X, X]),
                "group_1_term": lambda: pauli_sum(q, group1),
                "group_32_terms": lambda: pauli_sum(q, group32),
            }
        else:
            fns = {}
            if args.mode in ("per-term", "both"):
                fns["per-term"] = lambda: per_term(q, terms)
            if args.mode in ("sum", "both"):
                fns["sum"] = lambda: pauli_sum(q, terms)
        for name, r in measure(fns, args.warmup, args.reps).items():
            extra = {}
            if args.mode == "yardstick":
                extra["state_read_bytes_per_s"] = state_bytes / r["median_s"]
            report(bench="pauli_sum", width=n, terms=len(terms), what=name, reps=args.reps,
                   warmup=args.warmup, state_bytes=state_bytes, **r, **extra)
        del q


if __name__ == "__main__":
    main()
