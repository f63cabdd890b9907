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

  python tools/krylov_bench.py eigen fp32 28 [outdir]     (profiler off)

appends one row to <outdir>/krylov_eigen.csv, behind
profiles/PROF_KRYLOV_EIGEN.md: the marginal step of lanczos_lowest_states at
two basis sizes and one restart (see eigen() below).

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


EIGEN_DIMS = (4, 8, 12, 16)
EIGEN_REPS = 5


def eigen(prec, n, outdir):
    """One row of <outdir>/krylov_eigen.csv: lanczos_lowest_states(nev=1,
    max_restarts=0) at dim 4, 8, 12, 16 gives the marginal step at mean basis
    size 6.5 and 14.5; the same call at dim 16 with one restart (keep = 2: the
    rotation and the steps 3..16) gives the restart, after the 14 steps are
    taken off at the step time interpolated to their mean basis size 9.5.
    Models at the bandwidth of the in-place pauli_rotation: a step at basis
    size j moves (3L - 1 + 3j + 5) states, the rotation 16 + 2. The marginal
    step of lanczos_tridiagonal is measured alongside."""
    assert os.environ.get("QRACK_PROFILE") != "1"
    assert qa.hip_device_count() > 0, "needs the GPU"
    terms = heisenberg(n)
    L = launches(n)
    state_bytes = (8 if prec == "fp32" else 16) << n
    q = prepared(n, prec)

    def rmw():
        q.pauli_rotation([0, 1], [1, 3], 0.3)
        q.finish()

    def run(dim, restarts):
        def fn():
            _, _, info = q.lanczos_lowest_states(terms, 1, dim, 0.0, restarts)
            assert info["restarts"] == restarts and info["applies"] == dim + restarts * (dim - 2)
        return fn

    def plain(dim):
        return lambda: q.lanczos_tridiagonal(terms, dim)

    rmw()
    rmw_ms = med([clock(rmw) for _ in range(2 * REPS)])[0]
    bw = 2 * state_bytes / rmw_ms / 1e6  # GB/s
    calls = [run(d, 0) for d in EIGEN_DIMS] + [run(16, 1), plain(SHORT), plain(LONG)]
    # every call allocates and frees its own buffers, and calls of different
    # sizes taken in turn showed outliers of several hundred ms at 26 and 28
    # qubits (the per-call allocation PROF_KRYLOV.md names); the samples of
    # one call are therefore taken in a row, after a warm-up of that call
    samples = []
    for fn in calls:
        fn()
        samples.append([clock(fn) for _ in range(EIGEN_REPS)])
    t4, t8, t12, t16, t16r, p_short, p_long = [med(s)[0] for s in samples]
    spread = max((med(s)[2] - med(s)[1]) / med(s)[0] for s in samples)
    step_lo, step_hi = (t8 - t4) / 4, (t16 - t12) / 4
    slope = (step_hi - step_lo) / 8
    rotate = t16r - t16 - 14 * (step_lo + slope * (9.5 - 6.5))
    plain_step = (p_long - p_short) / (LONG - SHORT)
    unit = state_bytes / bw / 1e6  # ms per state size moved

    def model(j):
        return (3 * L - 1 + 3 * j + 5) * unit

    row = [prec, n, L, f"{rmw_ms:.3f}", f"{bw:.0f}", f"{t4:.2f}", f"{t8:.2f}", f"{t12:.2f}", f"{t16:.2f}",
           f"{t16r:.2f}", f"{spread:.3f}", f"{step_lo:.2f}", f"{model(6.5):.2f}", f"{step_lo / model(6.5):.3f}",
           f"{step_hi:.2f}", f"{model(14.5):.2f}", f"{step_hi / model(14.5):.3f}", f"{rotate:.2f}",
           f"{18 * unit:.2f}", f"{rotate / (18 * unit):.3f}", f"{plain_step:.2f}", f"{step_lo / plain_step:.3f}"]
    path = os.path.join(outdir, "krylov_eigen.csv")
    new = not os.path.exists(path)
    with open(path, "a", newline="") as f:
        wr = csv.writer(f)
        if new:
            wr.writerow(["precision", "qubits", "launches_L", "rmw_pass_ms", "rmw_GB_per_s", "call_dim4_ms",
                         "call_dim8_ms", "call_dim12_ms", "call_dim16_ms", "call_dim16_one_restart_ms",
                         "largest_relative_spread", "step_at_j6.5_ms", "model_ms", "step_over_model",
                         "step_at_j14.5_ms", "model_ms", "step_over_model", "rotate_k16_kp2_ms", "model_ms",
                         "rotate_over_model", "lanczos_tridiagonal_step_ms", "step_at_j6.5_over_tridiagonal_step"])
        wr.writerow(row)
    print(" ".join(str(x) for x in row), flush=True)


if __name__ == "__main__":
    out = sys.argv[4] if len(sys.argv) > 4 else "profiles"
    os.makedirs(out, exist_ok=True)
    {"step": step, "eigen": eigen}[sys.argv[1]](sys.argv[2], int(sys.argv[3]), out)
