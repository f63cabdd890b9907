"""Permutation ALU of the CPU engine, and of the layers that forward the
controlled modular ops to an engine, against the numpy oracle in
alu_oracle.py. Case table and checks: alu_cases.py.

The ALU only moves amplitudes (or negates them), so every case asserts
bit-for-bit equality with the oracle and |norm^2 - 1| <= 8 eps_R; the
carry-set cases marked `rescaled` get 4 eps (alu_cases.check_result).

Before the controlled multiply family cleared the controlled subspace of its
new vector, the cmul, cdiv, cmul_mod_n_out and cpow_mod_n_out cases here came
back with norm^2 between 1.15 and 1.57 on the random states and exactly 2.0
on the basis-state probes, on both engines: every controlled source slot that
was nobody's destination kept its amplitude.

Forwarding layers: QUnit forwards cmul_mod_n_out and cpow_mod_n_out, the C
API forwards mcmuln and mcpown, the pinvoke-compatible surface forwards
MCMUL, MCMULN and MCPOWN; each has a case below. QPager implements none of
the controlled multiply family.
"""

import ctypes
import glob
import os

import numpy as np
import pytest

import qrack_amd as qa
import alu_cases as ac
import alu_oracle as ao


def make(n, precision, layers=None):
    if layers:
        return qa.create_simulator(n, precision=precision, layers=layers, seed=7)
    return qa.create_simulator(n, precision=precision, engine="cpu", seed=7)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("case", ac.BASE_CASES, ids=ac.case_ids(ac.BASE_CASES))
def test_alu_vs_oracle(case, precision):
    ac.run_case(make(case.n, precision), case, precision)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("case", ac.WIDE_CASES, ids=ac.case_ids(ac.WIDE_CASES))
def test_alu_vs_oracle_13_qubits(case, precision):
    ac.run_case(make(case.n, precision), case, precision)


# ---- the basis-state probes that showed the duplicated amplitude ---------------

PROBES = [
    # (n, basis state, method, args, index after the op)
    (7, 3 | 1 << 6, "cmul", (5, 0, 3, 3, [6]), 7 | 1 << 3 | 1 << 6),
    (9, 2 | 1 << 8, "cpow_mod_n_out", (7, 15, 0, 4, 4, [8]), 2 | 4 << 4 | 1 << 8),
    (9, 6 | 1 << 8, "cmul_mod_n_out", (7, 15, 0, 4, 4, [8]), 6 | 12 << 4 | 1 << 8),
]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("probe", PROBES, ids=[p[2] for p in PROBES])
def test_controlled_op_moves_a_basis_state(probe, precision):
    """One basis state in, one basis state out: the source slot must not
    keep a copy of the amplitude (norm^2 was 2.0 before the fix)."""
    n, perm, method, args, moved = probe
    q = make(n, precision)
    q.set_permutation(perm)
    getattr(q, method)(*args)
    sv = np.asarray(q.get_state_vector())
    assert list(np.flatnonzero(sv)) == [moved]
    assert abs(sv[moved]) == 1.0
    start = np.zeros(1 << n, dtype=np.complex128)
    start[perm] = 1.0
    assert np.array_equal(np.abs(getattr(ao, method)(start, *args)), np.abs(sv))


# ---- layers that forward the controlled ops to an engine ----------------------

FORWARDED = [c for c in ac.BASE_CASES if c.id in ("cmul_mod_n_out-n15-c0-c9", "cpow_mod_n_out-n15-c0-c9")]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("case", FORWARDED, ids=ac.case_ids(FORWARDED))
def test_qunit_forwards_controlled_mod_ops(case, precision):
    """QUnit entangles the registers and the controls into one engine,
    remaps the controls and forwards; the reordering only swaps qubits."""
    ac.run_case(make(case.n, precision, layers=["qunit", "cpu"]), case, precision)


_SO = glob.glob(
    os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qrack_amd", "_qrack*.so")
)[0]
u64 = ctypes.c_uint64


def _arr(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(_SO)
    lib.qrack_init_count_type.restype = ctypes.c_uint64
    return lib


def _capi_run(lib, n, state, call):
    """Load a complex64 state into a plain CPU-engine simulator of the C
    API, run `call(sid)`, return the state."""
    sid = lib.qrack_init_count_type(n, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert sid != 0
    ket = np.ascontiguousarray(state.astype(np.complex64)).view(np.float32)
    buf = (ctypes.c_float * ket.size)(*ket)
    lib.InKet(u64(sid), buf)
    call(u64(sid))
    assert lib.qrack_get_error(u64(sid)) == 0
    out = (ctypes.c_float * ket.size)()
    lib.OutKet(u64(sid), out)
    lib.qrack_destroy(u64(sid))
    return np.array(out[:], dtype=np.float32).view(np.complex64)


# (id, oracle op, oracle args, C call); registers: in 1..4, out/carry 5..8, controls 0 and 9
_IN, _OUT, _CT = [1, 2, 3, 4], [5, 6, 7, 8], [0, 9]
C_CALLS = [
    (
        "capi-mcmuln",
        "cmul_mod_n_out",
        (7, 15, 1, 5, 4, _CT),
        lambda lib, s: lib.qrack_mcmuln(s, u64(7), _arr(_CT), u64(2), u64(15), u64(1), u64(5), u64(4)),
    ),
    (
        "capi-mcpown",
        "cpow_mod_n_out",
        (7, 15, 1, 5, 4, _CT),
        lambda lib, s: lib.qrack_mcpown(s, u64(7), u64(15), u64(1), u64(5), u64(4), _arr(_CT), u64(2)),
    ),
    (
        "pinvoke-MCMUL",
        "cmul",
        (5, 1, 5, 4, _CT),
        lambda lib, s: lib.MCMUL(s, u64(1), _arr([5]), u64(2), _arr(_CT), u64(4), _arr(_IN), _arr(_OUT)),
    ),
    (
        "pinvoke-MCMULN",
        "cmul_mod_n_out",
        (7, 13, 1, 5, 4, _CT),
        lambda lib, s: lib.MCMULN(
            s, u64(1), _arr([7]), u64(2), _arr(_CT), _arr([13]), u64(4), _arr(_IN), _arr(_OUT)
        ),
    ),
    (
        "pinvoke-MCPOWN",
        "cpow_mod_n_out",
        (7, 15, 1, 5, 4, _CT),
        lambda lib, s: lib.MCPOWN(
            s, u64(1), _arr([7]), u64(2), _arr(_CT), _arr([15]), u64(4), _arr(_IN), _arr(_OUT)
        ),
    ),
]


@pytest.mark.parametrize("entry", C_CALLS, ids=[e[0] for e in C_CALLS])
def test_c_abi_forwards_controlled_ops(lib, entry):
    """The C API and the pinvoke-compatible surface move their registers
    into place with swaps and forward to the engine."""
    name, op, args, call = entry
    case = ac.Case(name, 10, op, args, ac.reg(5, 4))
    state = ac.case_input(case, "fp32")
    got = _capi_run(lib, 10, state, lambda sid: call(lib, sid))
    ac.check_result(got, ac.case_expected(case, state), "fp32")
