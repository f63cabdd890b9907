"""QFT kernels of the HIP engine against the numpy oracle in qft_oracle.py:
qft / iqft over the case table of qft_cases.py (Gaussian and pending-basis
inputs, sub-registers, the pager over the engine, qftr) and the ramp
primitives. Table, derived tolerance and its condition: qft_cases.py, shared
with test_qft_oracle_cpu.py.

The default-switch table runs in-process on one engine per (width,
precision). One fresh child per switch setting (the switches are read once
per process) runs under QRACK_PROFILE=1, writes its states to an .npz and
fails at once if a case takes other host routes than its hand-written plan
declares; the parent holds the states to the oracle.

Tolerance. fp64: the derived C = 18 of qft_cases.py. fp32: every kernel
takes __sincosf, whose error has no documented bound, so C is measured:
FP32_MEASURED = 2.112 P eps (phase_ramp, case ramp-rs3-c0-m, element-wise;
the largest 2-norm figure is 1.038, n12-basis-ones iqft), the largest ratio
to the oracle over all 301 fp32 runs on an MI355X, and C_FP32 = 4 x that =
8.448. FP32_FAMILY holds the figures per kernel family. The fp64 runs stay
below 0.59 (2-norm) and 1.23 (element-wise) against the derived 18.
With C_FP32 the dropped-term floor of the flagged fp32 cases is 29 (length
13) to 4e5 times the tolerance. The unflagged ones still detect the removal
of every term of the top column up to 16 qubits (pi / 2^15), and from
control 1, 2, 3, 4, 5 upwards at 17, 18, 19, 20, 21 qubits: any term of angle
pi / 2^15 or more.

Kernel -> cases that reach it (hosts routes asserted by the children; the
kernel within a route read from its launcher):
- k_qft_col_v: n2, n13, n19 (c12.1) and every column of the fuse1 child
  (n10, n10-s3-l6 with rampStart 3); k_qft_col (fp64 only: an fp32 column
  above 0 always has tPow >= 2): fp64 n14, n12-s0-l4, fuse1 child.
- k_qft_col_v_pipe: pipe child (n10, nine columns).
- k_qft_col2 (scalar, tLo = 1): n6, n10 and all fp64 pairs; k_qft_col2_v:
  n10-s3-l6, fuse2 child. k_qft_col3 (scalar): n7, n11, fp64 n7;
  k_qft_col3_v: n10-s3-l7, n16-s5-l11, fuse3 child.
- k_qft_colK<4>: n6 to n11, the start > 0 cases, lds0 child (13-bit ramps);
  k_qft_colK<5>: fuse5 child (n10 twice in a row, n11, n12-s3-l8), both
  precisions.
- k_qft_low_lds: n12 to n21, n12-s0-l8, n12-s0-l4, n14-s0-l12 (four tiles),
  fp64 n11 to n14, n11-s0-l9, n11-s0-l6, n12-s0-l4 (K = 3, tile 2^11).
  k_qft_low_lds_var, basis: n12-basis-*, n14-s0-l12-basis-*,
  n16-s0-l14-basis-* iqft, fp64 n11-s0-l9-basis-*, n12-basis-* iqft,
  n13-basis-* iqft; tile sums: n23-dft.
- k_qft_mid_lds: n14, n16-s0-l14 (K = 2), n15, n18 (K = 3), n16 (K = 4),
  midmax6 child; k_qft_mid_lds_basis: n16-s0-l14-basis-* qft.
  k_qft_mid_wide: n17, n20 (8 columns), n21, n23-dft.
- support-restricted and sparse-last siblings: n14-basis-*, n17-basis-*,
  n21-basis-* (qft: mid support then sparse last; iqft: low support then
  mid support).
- later trips of the dense low, mid and wide tile loops and of the support
  ones: blocks3 child (n14 to n18, fp64 n13, n14, the basis cases).
- k_phase_ramp (condPower 1; fp64), k_phase_ramp_v, k_phase_ramp_gen and its
  host fallback above 8 relocated bits, k_qft_col_gen (target 0; fp64),
  k_qft_col_gen_v, k_qft_col2_gen, k_qft_col_top_range(_v): the primitives;
  PhaseRamp under the pager: pager-n16-s2-l13.

Sensitivity, shown on an MI355X with six mutations of a scratch build, one
at a time (a value or its attribution only, never an index, a bound, a grid
size or a loop limit). Failures of this file, then the verdict of the QFT
tests of the suite as it stood before (test_gpu.py, test_qft_lazy_gpu.py,
test_qft_sparse_last_gpu.py, test_qft_support_gpu.py, test_qft_wide_gpu.py,
test_dist_pager_gpu.py, test_engine_matrix.py; 160 GPU tests):
- launchQftColumnK's lowMask one bit short: 46 failures. Table cases n6,
  n7, n10, n11, n10-s3-l6, n10-s3-l7, n13-s1-l12, n16-s5-l11 (fp32), n7, n10,
  n12, n13, n14, n10-s3-l6, n13-s1-l12, six n12 / n13 basis cases and
  pager-n16 (fp64), and the fuse5, lds0, midlds0, midmax6, blocks3 and
  profile children. Before: fails (test_qft_fused2_numerics_vs_cpu).
- QEngineHIP::QFT passing rampStart = 0 to launchQftColumnK with start > 0:
  8 failures, the forward runs of n10-s3-l6, n10-s3-l7, n13-s1-l12,
  n16-s5-l11 (fp32), n10-s3-l6, n13-s1-l12 (fp64) and the fuse5 and profile
  children. Before: all 160 pass.
- launchQftMidLds's piSign without the sign when pre: 12 failures, iqft of
  n14, n15, n16, n18, n19, n16-s0-l14, two of its basis cases and pager-n16
  (fp32), and the midmax6, blocks3 and profile children. Before: fails
  (test_pager_qft_identity_prefix_on_hip).
- k_qft_low_lds's per-group scaleHi from gLo + K instead of gLo + K - 1: 53
  failures, every dense low-ladder case of both precisions (n12 to n21 and
  the shorter registers in fp32, n11 to n14 in fp64, pager-n16) and the
  fuse5, midlds0, midmax6, blocks3 and profile children. Before: fails
  (test_qft_fused2_numerics_vs_cpu).
- QEngineHIP::PhaseRampGeneral ignoring its last relocated weight: 16
  failures, every rampgen-k2-* and rampgen-k8-* primitive in both
  precisions (k0 has no relocated bit, k9 takes the host fallback).
  Before: all 160 pass.
- launchQftColumn2's scaleHi halved: 12 failures, fp64 n11, n12 and four
  n12 basis cases, and the fuse2, fuse5, midlds0 and profile children (the
  fp32 default schedules reach a column pair only as columns 1 and 0, whose
  ramp is empty). Before: fails (test_first_pass_from_basis_state[f64_n12]).
So two of the six passed every earlier QFT test; for the other four the
earlier run was stopped at its first failure, the test named.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import qft_cases as qc
import qft_oracle as qo

pytestmark = pytest.mark.gpu

# Measured on an MI355X over every fp32 case of the table, the primitives and
# the switch children (301 runs), each against the oracle, in units of
# P * eps_fp32: the largest figure is the element-wise 2.112 of the
# phase_ramp primitive (ramp-rs3-c0-m and ramp-rs3-c512-m: scale -pi / 32,
# rampStart 3); the largest 2-norm is 1.038 (n12-basis-ones iqft). Every kernel
# takes __sincosf, whose error depends on the angle, and the table samples
# few, so the tolerance is four times the measured value.
FP32_MEASURED = 2.112
FP32_MEASURED_CASE = "ramp-rs3-c0-m"
C_FP32 = 4 * FP32_MEASURED
# (2-norm, element-wise) per kernel family, same units, same run
FP32_FAMILY = {
    "register columns (col_v, col2/3 scalar and _v, colK<4>)": (0.668, 1.089),
    "FUSE=1 (col_v alone)": (0.249, 0.314),
    "FUSE=1 PIPE=1 (col_v_pipe)": (0.249, 0.297),
    "FUSE=2 / FUSE=3": (0.454, 0.724),
    "FUSE=5 (colK<5>)": (0.997, 1.962),
    "LDS=0 (13-bit register ramps)": (0.662, 1.041),
    "low ladder": (0.638, 0.935),
    "mid pass, 64-wide, and low ladder": (0.664, 0.909),
    "wide mid pass and low ladder": (0.680, 0.962),
    "23 qubits, tile-sums low ladder": (0.522, 0.675),
    "MIDLDS=0 / MIDMAX=6": (0.586, 0.933),
    "BLOCKS=3 (later trips of the tile loops)": (0.961, 1.893),
    "pending basis state (lazy first pass, support, sparse last)": (1.038, 2.057),
    "pager over the engine": (0.547, 0.738),
    "qftr (gate lowering)": (0.290, 0.451),
    "phase_ramp": (0.828, 2.112),
    "phase_ramp_general": (0.891, 2.026),
    "qft_column_general": (0.641, 1.431),
    "qft_column2_general": (0.763, 1.834),
    "qft_column_top_range (units of the page's norm)": (0.767, 1.647),
}


def c_of(precision):
    return C_FP32 if precision == "fp32" else qc.C_DERIVED


def _need_long(precision):
    if precision == "fp64" and not qo.LONG_OK:
        pytest.skip(qc.LONG_SKIP)


# One engine per (width, precision, layers) for the whole table, on purpose:
# every kernel also runs on an engine that has run the others, and a pending
# basis state follows a dense one on the same buffer.
_sims = {}


def make(n, precision, layers=()):
    assert qa.hip_device_count() > 0, "HIP engine must be present on GPU box (no silent fallback)"
    key = (n, precision, tuple(layers))
    if key not in _sims:
        if layers:
            _sims[key] = qa.create_simulator(n, precision=precision, seed=7,
                                             layers=list(layers) + ["hip"],
                                             pages_per_device=qc.PAGES_PER_DEVICE)
        else:
            _sims[key] = qa.create_simulator(n, precision=precision, engine="hip", seed=7)
    return _sims[key]


def _params(table):
    return [pytest.param(p, c, op, id=f"{c.id}-{op}-{p}")
            for p in qc.PRECISIONS for c in table(p) for op in c.ops]


@pytest.mark.parametrize("precision,case,op", _params(lambda p: qc.TABLE[p] + qc.PAGER_CASES))
def test_hip_engine_vs_oracle(precision, case, op):
    _need_long(precision)
    q = make(case.n, precision, case.layers or ())
    got = qc.run(q, case, op, precision)
    c = c_of(precision)
    qc.check(got, qc.expected(case, op, precision), precision, case.length, c=c,
             label=f"{case.id} {op}")
    if qc.full_ladder(case, precision):
        qc.check_floor(case, op, precision, c)
    elif case.basis is None and case.qubits is None and not case.dft_ref and case.n <= 17 \
            and case.length >= 2:
        print(f"{case.id} {op}: lowest control of the top column whose removal is detected: "
              f"{qc.detectable_ctrl(case, op, precision, c)}")


@pytest.mark.parametrize("precision", qc.PRECISIONS)
@pytest.mark.parametrize("prim_id", [p.id for p in qc.PRIMS])
def test_hip_primitive_vs_oracle(prim_id, precision):
    _need_long(precision)
    prim = qc.PRIM_BY_ID[prim_id]
    got = qc.run_prim(make(prim.n, precision), prim, precision)
    qc.check(got, qc.prim_expected(prim_id, precision), precision, prim.cols,
             c=c_of(precision), label=prim_id)


# ---- children: one process per switch setting ------------------------------------------

_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import numpy as np, qrack_amd as qa
import qft_cases as qc
assert qa.hip_device_count() > 0
mode, out_npz = sys.argv[3], sys.argv[4]
_env, _kw, per = qc.SWITCHES[mode]
sims, out = {}, {}
for precision in qc.PRECISIONS:
    for case in per[precision]:
        for op in case.ops:
            key = (case.n, precision)
            if key not in sims:
                sims[key] = qa.create_simulator(case.n, precision=precision, engine="hip", seed=7)
            qc.load(sims[key], case, precision)
            qa.profile_reset()
            qc.apply(sims[key], case, op)
            report = qa.profile_report()
            out[f"{case.id}/{op}/{precision}"] = np.asarray(sims[key].get_state_vector())
            seen = {o: int(report[o][0]) for o in qc.ROUTE_OPS if o in report}
            want = qc.routes_of(case.plan)
            assert seen == want, f"{mode} {case.id} {op} {precision}: took {seen}, declared {want}"
np.savez(out_npz, **out)
print("OK")
"""


def _run_child(tmp_path, mode):
    tests = os.path.dirname(os.path.abspath(__file__))
    out_npz = str(tmp_path / f"{mode}.npz")
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, os.path.dirname(tests),
           tests, mode, out_npz]
    env = {**os.environ, **qc.SWITCHES[mode][0], "QRACK_PROFILE": "1"}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stderr[-4000:])
    return np.load(out_npz)


def _check_switch(tmp_path, mode):
    got = _run_child(tmp_path, mode)
    for precision in qc.PRECISIONS:
        if precision == "fp64" and not qo.LONG_OK:
            continue
        for case in qc.SWITCHES[mode][2][precision]:
            for op in case.ops:
                qc.check(got[f"{case.id}/{op}/{precision}"], qc.expected(case, op, precision),
                         precision, case.length, c=c_of(precision),
                         label=f"{mode} {case.id} {op}")


def test_fuse_1_every_column_alone(tmp_path):
    """QRACK_GPU_QFT_FUSE=1: ten columns through k_qft_col_v (fp32) /
    k_qft_col (fp64), from bit 0 and with rampStart = 3."""
    _check_switch(tmp_path, "fuse1")


def test_fuse_2_column_pairs(tmp_path):
    _check_switch(tmp_path, "fuse2")


def test_fuse_3_column_triples(tmp_path):
    _check_switch(tmp_path, "fuse3")


def test_fuse_5_five_column_kernel(tmp_path):
    """QRACK_GPU_QFT_FUSE=5: k_qft_colK<R, 5, *>, twice in a row, over a
    remainder, and with rampStart = 3."""
    _check_switch(tmp_path, "fuse5")


def test_pipelined_single_column(tmp_path):
    """QRACK_GPU_QFT_PIPE=1 with FUSE=1: every column through k_qft_col_v_pipe."""
    _check_switch(tmp_path, "pipe")


def test_no_low_ladder(tmp_path):
    """QRACK_GPU_QFT_LDS=0: register columns with ramps of up to 13 bits."""
    _check_switch(tmp_path, "lds0")


def test_no_mid_pass(tmp_path):
    _check_switch(tmp_path, "midlds0")


def test_six_at_a_time_schedule(tmp_path):
    """QRACK_GPU_QFT_MIDMAX=6: the schedule without the wide kernel."""
    _check_switch(tmp_path, "midmax6")


def test_later_trips_of_the_tile_loops(tmp_path):
    """QRACK_GPU_BLOCKS=3: the dense and support-restricted LDS launchers
    honour the block cap, so 4 low tiles, 16 to 64 mid tiles and 16 wide
    tiles are walked by three blocks: the stride the 30-qubit transform
    runs on (32768 blocks over up to 2^18 tiles)."""
    _check_switch(tmp_path, "blocks3")


def test_cases_take_their_declared_routes(tmp_path):
    """QRACK_PROFILE=1 over the default table up to 19 qubits: each case
    must show exactly the profile_report() op counts of its plan."""
    _check_switch(tmp_path, "profile")


# ---- the streamed top column ------------------------------------------------------------

_TOP_N = 12
_TOP_ARGS = (np.pi / 64, 0, 0b111, [1 << 5], [32], 0.3)

_TOP_RANGE_CHILD = """
import torch
torch.cuda.init()
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import numpy as np, qrack_amd as qa
import qft_cases as qc
n, out_npz = int(sys.argv[3]), sys.argv[4]
scale, rs, mask, pows, ws, phase0 = eval(sys.argv[5])
half = 1 << (n - 1)
sv = qc.gaussian_state("top-own", n, "fp32")
tmp = qc.gaussian_state("top-recv", n - 1, "fp32")
out = {}
for pre in (False, True):
    sign = -1 if pre else 1
    for recv_is_low in (False, True):
        q = qa.create_simulator(n, engine="hip", seed=1)
        q.set_state_vector(sv)
        t = torch.from_numpy(tmp).cuda()
        torch.cuda.synchronize()
        step = half // 4
        for c in range(4):
            lo, hi = c * step, (c + 1) * step
            q.qft_column_top_range(sign * scale, rs, mask, pows, ws, sign * phase0, pre,
                                   lo, hi, t.data_ptr() + lo * 8, recv_is_low, 0)
        q.finish()
        out[f"{int(pre)}{int(recv_is_low)}"] = np.asarray(q.get_state_vector())
np.savez(out_npz, **out)
print("OK")
"""


def test_top_range_column_vs_oracle(tmp_path):
    """qft_column_top_range in four streamed chunks (torch initialised
    first, as its callers do): the general column on a page whose other half
    is the received buffer, against the oracle's column."""
    tests = os.path.dirname(os.path.abspath(__file__))
    out_npz = str(tmp_path / "top.npz")
    args = repr(tuple(float(a) if isinstance(a, float) else a for a in _TOP_ARGS))
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-c", _TOP_RANGE_CHILD,
           os.path.dirname(tests), tests, str(_TOP_N), out_npz, args]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stderr[-4000:])
    got = np.load(out_npz)
    scale, rs, mask, pows, ws, phase0 = _TOP_ARGS
    half = 1 << (_TOP_N - 1)
    sv = qc.gaussian_state("top-own", _TOP_N, "fp32")
    tmp = qc.gaussian_state("top-recv", _TOP_N - 1, "fp32")
    for pre in (False, True):
        sign = -1 if pre else 1
        for recv_is_low in (False, True):
            page = sv.copy()
            if recv_is_low:
                page[:half] = tmp
            else:
                page[half:] = tmp
            exp = qo.qft_column_general(qo.work(page), _TOP_N - 1, sign * scale, rs, mask, pows,
                                        ws, sign * phase0, pre)
            g = got[f"{int(pre)}{int(recv_is_low)}"]
            # the assembled page is not a unit vector: errors scale with its norm
            unit = float(np.linalg.norm(page.astype(np.complex128))) * qc.EPS["fp32"]
            two, mx, _nrm = qc.errors(g, exp)
            print(f"top-range pre={pre} recv_is_low={recv_is_low}: 2-norm {two / unit:.3f}, "
                  f"max {mx / qc.EPS['fp32']:.3f}")
            assert two <= C_FP32 * unit
            assert mx <= C_FP32 * qc.EPS["fp32"]
