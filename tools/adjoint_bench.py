"""Measurements behind profiles/PROF_ADJOINT.md, on the HIP engine.

  QRACK_PROFILE=1 python tools/adjoint_bench.py launches [outdir]
      per-launch times of pauli_adjoint, pauli_braket, pauli_apply and the
      in-place pauli_evolve yardstick at 28 / 30 qubits fp32 and 27 / 29 fp64
      -> adjoint_launches.csv
  python tools/adjoint_bench.py gradient [outdir]      (profiler off)
      a whole gradient of a 30-rotation ansatz under the 28-qubit Heisenberg
      chain against the same gradient by parameter shift
      -> adjoint_gradient.csv

  rocprofv3 --pmc FETCH_SIZE -d DIR --output-format csv -- python tools/adjoint_bench.py counters
      (and again with WRITE_SIZE: the two do not fit one pass) one fused launch
      per mask and precision for the counter collector, no tracing

Every figure is the median of REPS calls after a warm-up, in one process; a
profile sample is a host clock between two stream synchronisations around one
launch. outdir defaults to profiles/.
"""
import csv
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

import qrack_amd as qa

OUT = sys.argv[2] if len(sys.argv) > 2 else "profiles"
REPS = 7


def prepared(n, prec):
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=1)
    for i in range(n):
        q.ry(0.3 + 0.1 * i, i)
    q.finish()
    return q


def sample(fn, names):
    """median per-launch ms of each profile name over REPS calls of fn, after a warm-up"""
    fn()
    per = {k: [] for k in names}
    for _ in range(REPS):
        qa.profile_reset()
        fn()
        rep = qa.profile_report()
        for k in names:
            cnt, ms = rep[k]
            per[k].append(ms / cnt)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in per.items()}


def launches():
    assert os.environ.get("QRACK_PROFILE") == "1"
    rows = []
    ident = [(1.0, [], [])]
    for prec, n in (("fp32", 28), ("fp32", 30), ("fp64", 27), ("fp64", 29)):
        q = prepared(n, prec)
        b = prepared(n, prec)
        b.rz(0.4, 0)
        top = n - 1
        state_bytes = (8 if prec == "fp32" else 16) << n
        masks = {
            "low": ([0, 1], [1, 3]),
            "high": ([top, top - 1], [3, 1]),
            "diag": ([0, top], [2, 2]),
        }
        for name, (qs, ps) in masks.items():
            # one trainable rotation over an identity observable: one launch of every kind
            r = sample(lambda: q.adjoint_gradient([("rot", qs, ps, 0.3)], ident),
                       ["pauli_adjoint", "pauli_evolve", "pauli_apply", "pauli_braket"])
            rows.append((prec, n, "pauli_adjoint", name, 4, *r["pauli_adjoint"]))
            rows.append((prec, n, "pauli_evolve", name, 2, *r["pauli_evolve"]))
            if name == "low":
                rows.append((prec, n, "pauli_apply", "first(identity)", 2, *r["pauli_apply"]))
                rows.append((prec, n, "pauli_braket", "identity(in-sweep)", 2, *r["pauli_braket"]))
            term = [(1.0, qs, ps)]
            r = sample(lambda: q.pauli_sum_braket(b, term), ["pauli_braket"])
            rows.append((prec, n, "pauli_braket", name + "(call)", 2, *r["pauli_braket"]))
            r1 = sample(lambda: q.pauli_sum_apply_into(term, b), ["pauli_apply"])
            rows.append((prec, n, "pauli_apply", "first:" + name, 2, *r1["pauli_apply"]))
        # accumulate launch: a two-group sum is a first launch plus one accumulate launch
        two = [(1.0, [2], [2]), (1.0, *masks["low"])]
        r2 = sample(lambda: q.pauli_sum_apply_into(two, b), ["pauli_apply"])
        r1 = sample(lambda: q.pauli_sum_apply_into(two[:1], b), ["pauli_apply"])
        acc = 2 * r2["pauli_apply"][0] - r1["pauli_apply"][0]
        rows.append((prec, n, "pauli_apply", "first:diag", 2, *r1["pauli_apply"]))
        rows.append((prec, n, "pauli_apply", "accumulate:low(2 x pair median - first)", 3, acc, acc, acc))
        two = [(1.0, [2], [2]), (1.0, *masks["high"])]
        r2 = sample(lambda: q.pauli_sum_apply_into(two, b), ["pauli_apply"])
        acc = 2 * r2["pauli_apply"][0] - r1["pauli_apply"][0]
        rows.append((prec, n, "pauli_apply", "accumulate:high(2 x pair median - first)", 3, acc, acc, acc))
        del q, b
    with open(os.path.join(OUT, "adjoint_launches.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["precision", "qubits", "profile_name", "case", "state_sizes_moved", "median_ms",
                    "min_ms", "max_ms", "GB_per_s_at_median"])
        for prec, n, name, case, s, med, lo, hi in rows:
            state_bytes = (8 if prec == "fp32" else 16) << n
            w.writerow([prec, n, name, case, s, f"{med:.4f}", f"{lo:.4f}", f"{hi:.4f}",
                        f"{s * state_bytes / med / 1e6:.0f}"])
            print(prec, n, name, case, f"{med:.3f} ms", f"{s * state_bytes / med / 1e6:.0f} GB/s")


def heisenberg(n):
    return [(1.0, [b, b + 1], [p, p]) for b in range(n - 1) for p in (1, 3, 2)]


def gradient():
    assert os.environ.get("QRACK_PROFILE") != "1"
    n, prec = 28, "fp32"
    terms = heisenberg(n)
    rng = np.random.default_rng(3)
    theta = rng.uniform(-1, 1, size=30)
    ops = [("rot", [i], [3], float(theta[i])) for i in range(15)] \
        + [("rot", [i, i + 1], [2, 2], float(theta[15 + i])) for i in range(15)]
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=1)
    rows = []

    def adjoint():
        q.set_permutation(0x5555555)
        t0 = time.perf_counter()
        e, g = q.adjoint_gradient(ops, terms)
        q.finish()
        return (time.perf_counter() - t0) * 1e3, e, g

    adjoint()
    times = []
    for _ in range(REPS):
        ms, e, g = adjoint()
        times.append(ms)
    rows.append(("adjoint_gradient", statistics.median(times), min(times), max(times), 3 * 30 + 28))

    def energy(shifted):
        q.set_permutation(0x5555555)
        for op in shifted:
            q.pauli_rotation(op[1], op[2], op[3])
        return q.expectation_pauli_sum(terms)

    energy(ops)  # warm-up

    def shift():
        t0 = time.perf_counter()
        out = []
        for k in range(len(ops)):
            vals = []
            for sign in (+1, -1):
                op = ops[k]
                moved = ops[:k] + [(op[0], op[1], op[2], op[3] + sign * np.pi / 4)] + ops[k + 1:]
                vals.append(energy(moved))
            out.append(vals[0] - vals[1])
        return (time.perf_counter() - t0) * 1e3, np.array(out)

    times = []
    for _ in range(3):
        ms, gs = shift()
        times.append(ms)
    rows.append(("parameter_shift", statistics.median(times), min(times), max(times), 2 * 30 * (30 + 28)))
    # forward circuit + energy alone, for scale
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        energy(ops)
        times.append((time.perf_counter() - t0) * 1e3)
    rows.append(("circuit_plus_energy", statistics.median(times), min(times), max(times), 30 + 28))
    print("energy", e, "max |adjoint - shift| =", float(np.abs(g - gs).max()), "max |g| =", float(np.abs(g).max()))
    with open(os.path.join(OUT, "adjoint_gradient.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["what", "median_ms", "min_ms", "max_ms", "model_sweeps"])
        for name, med, lo, hi, sweeps in rows:
            w.writerow([name, f"{med:.2f}", f"{lo:.2f}", f"{hi:.2f}", sweeps])
            print(name, f"{med:.2f} ms", sweeps, "sweeps in the model")
        w.writerow(["max_abs_adjoint_minus_shift", f"{float(np.abs(g - gs).max()):.3e}", "", "", ""])


def counters():
    for prec, n in (("fp32", 28), ("fp64", 27)):
        q = prepared(n, prec)
        for qs, ps in (([0, 1], [1, 3]), ([n - 1, n - 2], [3, 1]), ([0, n - 1], [2, 2])):
            q.adjoint_gradient([("rot", qs, ps, 0.3)], [(1.0, [], [])])
        del q


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    {"launches": launches, "gradient": gradient, "counters": counters}[sys.argv[1]]()
