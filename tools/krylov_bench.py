"""Measurements behind profiles/PROF_KRYLOV.md, on the HIP engine. One
invocation measures one (precision, width) in a process of its own:

  python tools/krylov_bench.py step fp32 28 [outdir]      (profiler off)

appends one row to <outdir>/krylov_step.csv, for the Heisenberg chain (L = n
launches of H):

  * the in-place pauli_rotation that serves as the read-modify-write
    yardstick (2 state sizes of traffic) and the bandwidth it gives;
  * a whole lanczos_tridiagonal(dim) at dim = SHORT and dim = LONG, from which
    the marginal step, (t_LONG - t_SHORT) / (LONG - SHORT), and the fixed cost
    of a call (its norm reduction, the allocation and release of its three
    buffers), t_SHORT - SHORT * marginal, follow;
  * the same step composed from the public calls that existed before:
    pauli_sum_apply_into, expectation_pauli_sum and pauli_sum_braket with an
    identity term for the two overlaps. The two axpys have no public call and
    are left out, so the composed figure is a lower bound. Its three
    simulators live across calls: it has no per-call allocation.

Every figure is the median of REPS samples after a warm-up, a host clock
around work that ends in a stream synchronisation; the fused and the composed
samples are taken alternately. outdir defaults to profiles/.
"""
import csv
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import qrack_amd as qa

SHORT, LONG = 4, 12
REPS = 7


def heisenberg(n):
    return [(1.0, [b, b + 1], [p, p]) for b in range(n - 1) for p in (1, 3, 2)]


def launches(n):
    return n  # n - 1 bonds with an XX + YY group each, and one diagonal group


def prepared(n, prec):
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=1)
    for i in range(n):
        q.ry(0.3 + 0.1 * i, i)
    q.finish()
    return q


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def step(prec, n, outdir):
    assert os.environ.get("QRACK_PROFILE") != "1"
    assert qa.hip_device_count() > 0, "needs the GPU"
    terms = heisenberg(n)
    L = launches(n)
    state_bytes = (8 if prec == "fp32" else 16) << n
    q = prepared(n, prec)
    v_prev, w = prepared(n, prec), prepared(n, prec)
    ident = [(1.0, [], [])]

    def rmw():
        q.pauli_rotation([0, 1], [1, 3], 0.3)
        q.finish()

    def fused(dim):
        return lambda: q.lanczos_tridiagonal(terms, dim)

    def composed():
        # w = H v, alpha = <v|H|v>, <v_prev|w> and <w|w> through the identity braket
        q.pauli_sum_apply_into(terms, w)
        q.expectation_pauli_sum(terms)
        w.pauli_sum_braket(v_prev, ident)
        w.pauli_sum_braket(w, ident)
        q.finish()

    rmw()
    rmw_ms = med([clock(rmw) for _ in range(2 * REPS)])[0]
    bw = 2 * state_bytes / rmw_ms / 1e6  # GB/s
    for fn in (fused(SHORT), fused(LONG), composed):
        fn()
    t_short, t_long, t_comp = [], [], []
    for _ in range(REPS):
        t_short.append(clock(fused(SHORT)))
        t_comp.append(clock(composed))
        t_long.append(clock(fused(LONG)))
        t_comp.append(clock(composed))
    s_med, s_lo, s_hi = med(t_short)
    l_med, l_lo, l_hi = med(t_long)
    c_med, c_lo, c_hi = med(t_comp)
    marginal = (l_med - s_med) / (LONG - SHORT)
    fixed = s_med - SHORT * marginal
    model_ms = (3 * L + 3) * state_bytes / bw / 1e6
    row = [prec, n, L, f"{rmw_ms:.3f}", f"{bw:.0f}",
           f"{s_med:.2f}", f"{s_lo:.2f}", f"{s_hi:.2f}", f"{l_med:.2f}", f"{l_lo:.2f}", f"{l_hi:.2f}",
           f"{marginal:.2f}", f"{fixed:.2f}", f"{model_ms:.2f}", f"{marginal / model_ms:.3f}",
           f"{c_med:.2f}", f"{c_lo:.2f}", f"{c_hi:.2f}", f"{c_med / marginal:.3f}",
           f"{c_med / (s_med / SHORT):.3f}"]
    path = os.path.join(outdir, "krylov_step.csv")
    new = not os.path.exists(path)
    with open(path, "a", newline="") as f:
        wr = csv.writer(f)
        if new:
            wr.writerow(["precision", "qubits", "launches_L", "rmw_pass_ms", "rmw_GB_per_s",
                         f"call_dim{SHORT}_ms", "min_ms", "max_ms", f"call_dim{LONG}_ms", "min_ms", "max_ms",
                         "marginal_step_ms", "fixed_per_call_ms", "model_step_ms_at_rmw_bandwidth",
                         "marginal_over_model", "composed_step_ms_without_axpys", "min_ms", "max_ms",
                         "composed_over_marginal", f"composed_over_dim{SHORT}_call_per_step"])
        wr.writerow(row)
    print(" ".join(str(x) for x in row), flush=True)


if __name__ == "__main__":
    out = sys.argv[4] if len(sys.argv) > 4 else "profiles"
    os.makedirs(out, exist_ok=True)
    {"step": step}[sys.argv[1]](sys.argv[2], int(sys.argv[3]), out)
