"""Permutation ALU of the HIP engine (k_permute, k_copy_uncontrolled,
k_phaseflipless) against the numpy oracle in alu_oracle.py. Case table and
checks: alu_cases.py, shared with test_alu_oracle_cpu.py.

Every case asserts bit-for-bit equality with the oracle and
|norm^2 - 1| <= 8 eps_R. The only exception is the set of cases marked
`rescaled` in the table (a set carry qubit is measured and collapsed before
the permutation: QEngine::ForceM in csrc/qengine.hpp scales by
1/sqrt(prob) through k_applym; see alu_cases.check_result), which get
4 eps elementwise. Measured on an MI355X: those cases are off by at most
1.33 eps in fp64 and by nothing in fp32; every other case is bit for bit.
SetQuantumState leaves runningNorm = -1, but no ALU path normalises: only
Dispose and Decompose call NormalizeState.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import alu_cases as ac

pytestmark = pytest.mark.gpu


def make(n, precision):
    assert qa.hip_device_count() > 0, "HIP engine must be present on GPU box (no silent fallback)"
    return qa.create_simulator(n, precision=precision, engine="hip", seed=7)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("case", ac.BASE_CASES, ids=ac.case_ids(ac.BASE_CASES))
def test_alu_vs_oracle(case, precision):
    ac.run_case(make(case.n, precision), case, precision)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("case", ac.WIDE_CASES, ids=ac.case_ids(ac.WIDE_CASES))
def test_alu_vs_oracle_13_qubits(case, precision):
    ac.run_case(make(case.n, precision), case, precision)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_controlled_op_moves_a_basis_state(precision):
    """cmul on one basis state: the source slot must not keep a copy."""
    q = make(7, precision)
    q.set_permutation(3 | 1 << 6)
    q.cmul(5, 0, 3, 3, [6])
    sv = np.asarray(q.get_state_vector())
    assert list(np.flatnonzero(sv)) == [7 | 1 << 3 | 1 << 6]
    assert abs(sv[79]) == 1.0


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_table_ops_repeated_on_one_engine(precision):
    """The indexed ops and hash upload their table for every call, the way
    the multiplexer uploads its matrices; there, calls after the first on
    one engine intermittently read zeros in place of the upload. Every other
    test here makes a new engine per case, so: three rounds of the table
    cases on one engine."""
    cases = [c for c in ac.BASE_CASES if c.op in ("indexed_lda", "indexed_adc", "hash") and not c.rescaled]
    q = make(10, precision)
    for _ in range(3):
        for case in cases:
            ac.run_case(q, case, precision)


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import numpy as np, qrack_amd as qa
import alu_cases as ac
assert qa.hip_device_count() > 0
out = {}
for precision in ("fp32", "fp64"):
    for case in ac.STRIDE_CASES:
        q = qa.create_simulator(case.n, precision=precision, engine="hip", seed=7)
        out[case.id + "/" + precision] = ac.apply_case(q, case, ac.case_input(case, precision), precision)
np.savez(sys.argv[3], **out)
print("OK")
"""


def test_grid_stride_loop_under_block_cap(tmp_path):
    """gridFor launches an exact grid, so k_permute's stride loop only runs
    under QRACK_GPU_BLOCKS. The variable is read once per process: a fresh
    child runs inc, cmul_mod_n_out, indexed_adc and rol with two blocks for
    1024 amplitudes, and the parent compares with the oracle."""
    tests = os.path.dirname(os.path.abspath(__file__))
    out_npz = str(tmp_path / "stride.npz")
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, os.path.dirname(tests), tests, out_npz]
    r = subprocess.run(cmd, env={**os.environ, "QRACK_GPU_BLOCKS": "2"}, capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr
    got = np.load(out_npz)
    for precision in ("fp32", "fp64"):
        for case in ac.STRIDE_CASES:
            state = ac.case_input(case, precision)
            ac.check_result(got[case.id + "/" + precision], ac.case_expected(case, state), precision)
