"""Pauli-string and Pauli-sum expectation values: the one-pass CPU engine
path, the default lowering through the layers, validation, the C ABI and
the example.

Oracle: numpy float64 dense index arithmetic on the engine's own
get_state_vector(), which isolates the expectation pass from gate rounding.
Tolerance on |got - want| is 1e-6 * sum|c_t| (fp32) and 1e-12 * sum|c_t|
(fp64): the half-space products satisfy sum 2|psi_i||psi_j| <= 1 and each
carries a few ulp of the amplitude type; the sum itself is in double.
"""
import ctypes
import glob
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"fp32": 1e-6, "fp64": 1e-12}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}
WIDTHS = (1, 2, 3, 5, 9)


def strings_for(n, rng):
    if n <= 3:
        return [(list(range(n)), list(ps)) for ps in itertools.product(range(4), repeat=n)]
    return [po.random_string(n, rng) for _ in range(64)]


def engine_with_state(n, prec, seed, engine="cpu"):
    rng = np.random.default_rng(seed)
    q = qa.create_simulator(n, engine=engine, precision=prec, seed=1)
    q.set_state_vector(po.random_state(n, rng, DTYPE[prec]))
    return q, np.asarray(q.get_state_vector()), rng


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("n", WIDTHS)
def test_strings_and_sum_match_dense(n, prec):
    q, sv, rng = engine_with_state(n, prec, 100 + n)
    tol = TOL[prec]
    for qs, ps in strings_for(n, rng):
        want = po.expect(sv, qs, ps)
        assert abs(q.pauli_expectation(qs, ps) - want) <= tol, (qs, ps)
        assert abs(q.expectation_pauli_all(qs, ps) - want) <= tol, (qs, ps)
        # d(1 - E^2) = 2|E| dE <= 2 dE
        assert abs(q.variance_pauli_all(qs, ps) - (1 - want * want)) <= 2 * tol, (qs, ps)
    terms = po.random_terms(n, rng, 40)
    got = q.expectation_pauli_sum(terms)
    assert abs(got - po.expect_sum(sv, terms)) <= tol * po.abs_coeffs(terms)


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_state_is_untouched(prec):
    n = 5
    q, sv, rng = engine_with_state(n, prec, 7)
    before = sv.tobytes()
    qs, ps = [3, 0, 4, 1], [1, 3, 2, 3]
    terms = po.random_terms(n, rng, 12)
    for call in (
        lambda: q.pauli_expectation(qs, ps),
        lambda: q.expectation_pauli_all(qs, ps),
        lambda: q.variance_pauli_all(qs, ps),
        lambda: q.expectation_pauli_sum(terms),
    ):
        call()
        assert np.asarray(q.get_state_vector()).tobytes() == before


def entangle(q, n):
    for i in range(n):
        q.h(i)
        q.ry(0.2 + 0.3 * i, i)
    for i in range(n - 1):
        q.cnot(i, i + 1)
    for i in range(n):
        q.rz(0.15 * (i + 1), i)
    q.cnot(n - 1, 0)


@pytest.mark.parametrize(
    "layers",
    [["qunit", "cpu"], ["stabilizer_hybrid", "cpu"], ["pager", "cpu"], ["fuser", "cpu"], ["hybrid"]],
    ids=lambda l: "-".join(l),
)
def test_default_path_through_layers(layers):
    n = 6
    rng = np.random.default_rng(31)
    terms = po.random_terms(n, rng, 12)
    bare = qa.create_simulator(n, engine="cpu", seed=3)
    entangle(bare, n)
    want = bare.expectation_pauli_sum(terms)
    q = qa.create_simulator(n, layers=layers, seed=3)
    entangle(q, n)
    assert abs(q.expectation_pauli_sum(terms) - want) <= 1e-5


def test_validation_and_canonical_form():
    n = 4
    q, sv, _ = engine_with_state(n, "fp64", 9)
    with pytest.raises(Exception):
        q.expectation_pauli_sum([(1.0, [0, 0], [1, 2])])  # repeated qubit
    with pytest.raises(Exception):
        q.expectation_pauli_sum([(1.0, [n], [1])])  # out of range
    with pytest.raises(Exception):
        q.expectation_pauli_sum([(1.0, [0, 1], [1])])  # size mismatch
    # all-identity terms contribute exactly their coefficient
    assert q.expectation_pauli_sum([(0.375, [], [])]) == 0.375
    assert q.expectation_pauli_sum([(0.375, [2, 0], [0, 0])]) == 0.375
    assert q.expectation_pauli_sum([]) == 0.0
    # duplicate terms merge
    t = (0.7, [1, 3, 0], [1, 3, 2])
    once = q.expectation_pauli_sum([t])
    assert abs(once - 0.7 * po.expect(sv, t[1], t[2])) <= 1e-12
    assert abs(q.expectation_pauli_sum([t, t]) - 2 * once) <= 1e-12
    # identity factors are dropped before merging
    padded = (0.7, [1, 2, 3, 0], [1, 0, 3, 2])
    assert abs(q.expectation_pauli_sum([t, padded]) - 2 * once) <= 1e-12


def test_repeated_qubit_in_single_string_keeps_generic_answer():
    # Z then Z on one qubit: the generic lowering sees the mask of one Z
    q = qa.create_simulator(2, engine="cpu", seed=1)
    q.ry(0.8, 0)
    z = q.pauli_expectation([0], [2])
    assert abs(q.pauli_expectation([0, 0], [2, 2]) - z) <= 1e-6


def test_capi_bell_state():
    so = glob.glob(os.path.join(REPO, "qrack_amd", "_qrack*.so"))[0]
    lib = ctypes.CDLL(so)
    lib.qrack_init_count_type.restype = ctypes.c_uint64
    lib.qrack_expectation_pauli_sum.restype = ctypes.c_double
    u64 = ctypes.c_uint64
    sid = lib.qrack_init_count_type(2, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert sid != 0
    lib.qrack_h(u64(sid), u64(0))
    c = (ctypes.c_uint64 * 1)(0)
    lib.qrack_mcx(u64(sid), c, u64(1), u64(1))
    # Bell state: <XX> = 1, <YY> = -1, <ZZ> = 1, <Z0> = 0, identity = 1
    coeffs = (ctypes.c_double * 5)(0.5, 0.25, 2.0, 3.0, -1.0)
    lens = (ctypes.c_uint64 * 5)(2, 2, 2, 1, 0)
    qs = (ctypes.c_uint64 * 7)(0, 1, 0, 1, 0, 1, 0)
    ps = (ctypes.c_int * 7)(1, 1, 3, 3, 2, 2, 2)
    e = lib.qrack_expectation_pauli_sum(u64(sid), u64(5), coeffs, lens, qs, ps)
    assert abs(e - (0.5 - 0.25 + 2.0 + 0.0 - 1.0)) <= 1e-5
    assert lib.qrack_get_error(u64(sid)) == 0
    # a repeated qubit is reported through the error flag, not a crash
    bad_q = (ctypes.c_uint64 * 2)(1, 1)
    bad_p = (ctypes.c_int * 2)(1, 2)
    lib.qrack_expectation_pauli_sum(
        u64(sid), u64(1), (ctypes.c_double * 1)(1.0), (ctypes.c_uint64 * 1)(2), bad_q, bad_p)
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))


def test_example_runs():
    exdir = os.path.join(REPO, "examples")
    out = subprocess.run(
        [sys.executable, "pauli_sum_energy.py"],
        cwd=exdir, capture_output=True, text=True, timeout=300,
        env={**os.environ, "PYTHONPATH": REPO},
    )
    assert out.returncode == 0, f"{out.stdout}\n{out.stderr}"
    assert "OK" in out.stdout
