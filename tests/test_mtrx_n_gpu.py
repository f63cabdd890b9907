"""Dense k-qubit gates on the HIP engine (k_mtrx_n, and the delegations of
k = 1 and the uncontrolled k = 2) against gate_oracle.State.apply. Case table,
derived tolerance and checks: mtrx_n_cases.py, shared with test_mtrx_n_cpu.py.

The table runs in-process on one engine per (width, precision), so every case
also runs after other matrices on the same engine: a matrix that reaches the
kernel late or stale shows from the second call on. Two fresh children (the
switches are read once per process) cover QRACK_GPU_BLOCKS=2 over the 14-qubit
cases (the tile loop runs a second trip: 4 tiles in fp32, 8 in fp64, for two
workgroups) and QRACK_PROFILE=1 (each case must show exactly one op of the
route it declares). Each child writes its states to an .npz and the parent
holds them to the oracle.

Measured on an MI355X, the largest error over the table in G eps a
(fp32 / fp64): k = 1: 0.97 / 1.51, k = 2: 1.68 / 1.69, k = 3: 1.82 / 1.96,
k = 4: 1.69 / 2.16, k = 5: 2.06 / 2.49, k = 6: 2.03 / 2.21, against the derived
worst-case bounds 3, 3, 5, 9, 17, 33. The whole file runs in about 3 seconds
there.

Sensitivity, shown on an MI355X with two host-side mutations of a scratch
build (values or their attribution only, never an index); each fails here:
- QEngineHIP::MtrxN copies the matrix without the row and column
  permutation: 26 failures, every case whose targets are not ascending
  (two-n7-k6-q6_1_2_3_4_5, small-n10-k3-q9_0_5, tiles-n14-k3-q5_13_2,
  ctl-n14-k3-q11_9_10-a5_13, ctl-n14-k4-q3_2_1_0-a12_13, the diag, gauss and
  shift kinds on q5_13_2 and its controlled shift, basis-n10-k3-q2_0_7-perm5;
  both precisions), test_same_gate_twice_on_one_engine (both), the BLOCKS and
  PROFILE children and the fuser layer test (both). The identity on q5_13_2
  passes, as it must.
- QEngineHIP::MtrxN ignores `anti`: 60 failures, route-n14-k1-q12-a3_13,
  all 24 ctl-n10-* and ctl-n14-* anti-control cases,
  ctl-n14-k3-q11_9_10-a5_13 and ctl-n14-k4-q3_2_1_0-a12_13 (both precisions),
  the BLOCKS and PROFILE children and all four layer tests. The
  anti-controlled identity passes, as it must.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import gate_oracle as go
import mtrx_n_cases as mc
from gate_cases import DTYPE, _clist, _unitary

pytestmark = pytest.mark.gpu

_sims = {}


def make(n, precision):
    assert qa.hip_device_count() > 0, "HIP engine must be present on GPU box (no silent fallback)"
    key = (n, precision)
    if key not in _sims:
        _sims[key] = qa.create_simulator(n, precision=precision, engine="hip", seed=7)
    return _sims[key]


@pytest.mark.parametrize("precision", mc.PRECISIONS)
@pytest.mark.parametrize("case_id", mc.IDS)
def test_mtrx_n_vs_oracle(case_id, precision):
    case = mc.BY_ID[case_id]
    mc.run_case(make(case.n, precision), case, precision)


@pytest.mark.parametrize("precision", mc.PRECISIONS)
def test_same_gate_twice_on_one_engine(precision):
    """Two different 16 x 16 matrices through the aux buffer back to back, no
    read in between: the second upload must not overtake the first kernel."""
    n, qubits = 13, (12, 0, 5, 7)
    rng = np.random.default_rng(99)
    state = go.random_state(n, rng).astype(DTYPE[precision])
    q = make(n, precision)
    q.set_state_vector(state)
    st = go.State(state.astype(np.complex128))
    for _ in range(2):
        m = _clist(_unitary(rng, 16), precision)
        q.mtrx_n(list(qubits), m)
        st.apply(qubits, m)
    mc.check_state(np.asarray(q.get_state_vector()), st, precision, 4, "twice-n13-k4")


# ---- children: one process per switch ---------------------------------------------

_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import numpy as np, qrack_amd as qa
import mtrx_n_cases as mc
assert qa.hip_device_count() > 0
mode, out_npz = sys.argv[3], sys.argv[4]
cases = [c for c in mc.CASES if mode == "profile" or c.n == 14]
sims, out, wrong = {}, {}, []
for precision in mc.PRECISIONS:
    for case in cases:
        key = (case.n, precision)
        if key not in sims:
            sims[key] = qa.create_simulator(case.n, precision=precision, engine="hip", seed=7)
        mc.load_input(sims[key], case, precision)
        qa.profile_reset()
        sims[key].mtrx_n(list(case.qubits), mc.case_matrix(case, precision), list(case.controls),
                         case.anti)
        report = qa.profile_report()
        out[case.id + "/" + precision] = np.asarray(sims[key].get_state_vector())
        if mode == "profile":
            seen = {op: int(report[op][0]) for op in mc.ROUTE_OPS if op in report}
            if seen != {mc.route_of(case): 1}:
                wrong.append(f"{case.id}/{precision}: took {seen}, expected one {mc.route_of(case)}")
np.savez(out_npz, **out)
assert not wrong, "host routes differ from the table:\\n" + "\\n".join(wrong)
print("OK")
"""


def _run_child(tmp_path, mode, env):
    tests = os.path.dirname(os.path.abspath(__file__))
    out_npz = str(tmp_path / f"{mode}.npz")
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, os.path.dirname(tests),
           tests, mode, out_npz]
    r = subprocess.run(cmd, env={**os.environ, **env}, capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-4000:]
    return np.load(out_npz)


def test_second_trip_of_the_tile_loop_under_block_cap(tmp_path):
    """k_mtrx_n launches one workgroup per tile by default. With
    QRACK_GPU_BLOCKS=2 the 14-qubit cases give two workgroups 4 (fp32) or 8
    (fp64) tiles, fewer where a control outside the tile halves them."""
    got = _run_child(tmp_path, "stride", {"QRACK_GPU_BLOCKS": "2"})
    for precision in mc.PRECISIONS:
        for case in mc.CASES:
            if case.n == 14:
                mc.check_case(got[case.id + "/" + precision], case, precision)


def test_cases_take_their_declared_routes(tmp_path):
    """QRACK_PROFILE=1: after profile_reset() every case must show one
    `mtrx_n`, or one `apply2x2` for k = 1, or one `mtrx_2q` for the
    uncontrolled k = 2, and nothing else of the three. The states are held to
    the oracle as well."""
    got = _run_child(tmp_path, "profile", {"QRACK_PROFILE": "1"})
    for precision in mc.PRECISIONS:
        for case in mc.CASES:
            mc.check_case(got[case.id + "/" + precision], case, precision)


# ---- layers over the engine --------------------------------------------------------

@pytest.mark.parametrize("precision", mc.PRECISIONS)
@pytest.mark.parametrize("layer", ("fuser", "qunit"))
def test_layers_over_hip_vs_oracle(layer, precision):
    """Three mtrx_n calls mixed among 1q unitaries at 13 qubits, past the
    tile of both precisions: the fuser must flush its pending 2x2s before
    each call, QUnit must entangle what the call touches. Three 1q gates per
    call keep the oracle's a_i, and with it the bound, within about 10^3 |v_i|."""
    assert qa.hip_device_count() > 0
    n = 13
    rng = np.random.default_rng(4243)
    q = qa.create_simulator(n, precision=precision, layers=[layer, "hip"], seed=7)
    v = np.zeros(1 << n, dtype=np.complex128)
    v[0] = 1.0
    st = go.State(v)
    calls = [((12, 3, 0), (), False, (3, 12, 6)), ((1, 5, 6, 11), (3,), False, (0, 5, 9)),
             ((7, 4, 9, 10, 12), (0, 6), True, (6, 10, 2))]
    c_sum = 0
    for qubits, controls, anti, singles in calls:
        for t in singles:
            m = _clist(_unitary(rng, 2), precision)
            q.mtrx(m, t)
            st.mtrx(m, t)
            c_sum += mc.c_of_k(1)
        m = _clist(_unitary(rng, 1 << len(qubits)), precision)
        q.mtrx_n(list(qubits), m, list(controls), anti)
        st.apply(qubits, m, controls, anti)
        c_sum += mc.c_of_k(len(qubits))
    assert st.gates == 12
    got = np.asarray(q.get_state_vector())
    mc.check_state(got, st, precision, 5, f"{layer}-n{n}", c_sum=c_sum)
    # the bound must mean something: well below the amplitudes themselves
    nz = np.abs(st.v) > 0
    assert c_sum * mc.EPS[precision] * float(np.median(st.a[nz] / np.abs(st.v[nz]))) < 1e-3
