"""Multi-qubit reduced density matrices without a GPU: the pass planner, the
CPU engine, QUnit, the forwarding wrappers, the generic lowering, the Python
helpers, the C ABI and the example. Oracle and tolerance: rdm_oracle.py (the
CPU paths sum in double throughout, so E_R = 0).
"""
import ctypes
import glob
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import rdm_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("fp32", "fp64")
STATE_TOL = {"fp32": 2e-6, "fp64": 1e-12}  # gate rounding included


def cpu_with_state(n, prec, seed, layers=None):
    rng = np.random.default_rng(seed)
    q = qa.create_simulator(n, precision=prec, layers=layers or ["cpu"], seed=1)
    q.set_state_vector(ro.random_state(n, rng, ro.DTYPE[prec]))
    return q, np.asarray(q.get_state_vector())


# ---- planner -----------------------------------------------------------------------


@pytest.mark.parametrize("prec", PRECS)
def test_planner_regimes_and_launch_lists(prec):
    n = 12
    assert 1 <= qa.RDM_REG_MAX < qa.RDM_TILE_MAX < qa.RDM_MAX_QUBITS == 12
    assert 0 <= qa.RDM_RUN <= 64
    for k in range(1, 10):
        for kept in (list(range(k)), list(range(n - k, n)), [(5 * j + 3) % n for j in range(k)]):
            assert len(set(kept)) == k
            plan = qa.rdm_pass_plan(n, kept, prec)
            want = ("register" if k <= qa.RDM_REG_MAX
                    else "tile" if k <= qa.RDM_TILE_MAX else "wide")
            assert plan["regime"] == want, (k, kept)
            tile, block = plan["tile_bits"], plan["block_bits"]
            assert sorted(tile + block) == sorted(kept) and not set(tile) & set(block)
            if want == "wide":
                assert len(tile) == qa.RDM_TILE_MAX
                # the physically lowest kept bits stay in the tile
                assert max(tile) < min(block)
                nb = 1 << len(block)
                assert sorted(plan["launches"]) == [
                    (a, b) for a in range(nb) for b in range(a, nb)]
                assert len(plan["launches"]) == nb * (nb + 1) // 2
            else:
                assert block == [] and plan["launches"] == [(0, 0)]
    # the planner honours sets, not orders
    assert qa.rdm_pass_plan(n, [7, 2, 11], prec) == qa.rdm_pass_plan(n, [2, 7, 11], prec)
    for bad in ([], [1, 1], [12], list(range(13))):
        with pytest.raises(Exception):
            qa.rdm_pass_plan(13 if len(bad) == 13 else n, bad, prec)


# ---- CPU engine ----------------------------------------------------------------------

KEPT_10 = ([0], [9], [0, 9], [7, 2, 9], [2, 7, 9], list(range(10)), list(range(1, 10)))


@pytest.fixture(scope="module", params=PRECS)
def state10(request):
    q, sv = cpu_with_state(10, request.param, 1000)
    return request.param, q, sv


@pytest.mark.parametrize("kept", KEPT_10, ids=lambda k: "-".join(map(str, k)))
def test_cpu_engine_against_oracle(state10, kept):
    prec, q, sv = state10
    got = q.reduced_density_matrix(kept)
    ro.check(got, ro.rdm(sv, kept), prec, 0, kept)
    again = q.reduced_density_matrix(kept)
    assert got.tobytes() == again.tobytes()  # fixed fold order: bit-identical
    assert np.asarray(q.get_state_vector()).tobytes() == sv.tobytes()


def test_order_is_honoured(state10):
    prec, q, sv = state10
    a = q.reduced_density_matrix([7, 2, 9])
    b = q.reduced_density_matrix([2, 7, 9])
    assert not np.array_equal(a, b)
    # swapping bits 0 and 1 of the index maps one onto the other
    perm = [((i & 1) << 1) | ((i >> 1) & 1) | (i & 4) for i in range(8)]
    assert np.array_equal(a, b[np.ix_(perm, perm)])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2))
def test_cpu_engine_tiny_widths(n, prec):
    q, sv = cpu_with_state(n, prec, 10 + n)
    for k in range(1, n + 1):
        for kept in itertools.permutations(range(n), k):
            ro.check(q.reduced_density_matrix(list(kept)), ro.rdm(sv, kept), prec, 0, kept)


@pytest.mark.parametrize("layers", (["cpu"], ["qunit", "cpu"], ["sparse"]), ids="-".join)
def test_errors(layers):
    q = qa.create_simulator(14, layers=layers, seed=1)
    for bad in ([], [3, 3], [1, 14], [-1], list(range(13))):
        with pytest.raises(Exception):
            q.reduced_density_matrix(bad)
    assert q.reduced_density_matrix(list(range(12))).shape == (4096, 4096)


def test_single_qubit_form_is_the_k1_case(state10):
    prec, q, sv = state10
    for b in (0, 4, 9):
        one = np.asarray(q.reduced_density_matrix(b)).astype(np.complex128)
        lst = q.reduced_density_matrix([b])
        # the int form is rounded to the engine's precision on the way out
        assert np.all(np.abs(one - lst) <= ro.bound(ro.rdm(sv, [b]), prec, 0) + ro.EPS[prec] * np.abs(lst))


# ---- layers --------------------------------------------------------------------------


def three_units_and_a_buffered_cz(q):
    """(0,1,2) (3,4) (5,6) entangled inside, 7 alone; CZ(2,3) stays buffered."""
    for i in range(8):
        q.ry(0.3 + 0.2 * i, i)
    q.cnot(0, 1)
    q.cnot(1, 2)
    q.cnot(3, 4)
    q.cnot(5, 6)
    for i in range(8):
        q.rz(0.1 * (i + 1), i)
        q.ry(0.15 * (i + 2), i)
    q.cz(2, 3)
    return q


@pytest.mark.parametrize("prec", PRECS)
def test_qunit_kronecker_product(prec):
    q = three_units_and_a_buffered_cz(
        qa.create_simulator(8, precision=prec, layers=["qunit", "cpu"], seed=5))
    dense = three_units_and_a_buffered_cz(
        qa.create_simulator(8, precision=prec, layers=["cpu"], seed=5))
    sv = np.asarray(dense.get_state_vector())
    assert q.are_factorized([0, 1, 2, 3, 4], [5, 6]) and q.are_factorized([5, 6], [7])
    assert not q.are_factorized([0, 1, 2], [3, 4])  # the buffered CZ links them
    # [6, 0, 4] spans the three units and leaves the CZ buffered (it acts on
    # qubits that are traced out); [6, 0, 3, 2] has to land it first
    for kept in ([6, 0, 4], [6, 0, 3, 2], [4, 7, 1], [5], [3, 2]):
        got = q.reduced_density_matrix(kept)
        assert np.abs(got - ro.rdm(sv, kept)).max() <= STATE_TOL[prec], kept
        assert np.array_equal(got, q.reduced_density_matrix(kept)), kept


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layers", (["fuser", "cpu"], ["noisy", "cpu"]), ids="-".join)
def test_wrappers_reach_the_cpu_engine(layers, prec):
    def circuit(q):
        for i in range(9):
            q.ry(0.2 + 0.3 * i, i)
        for i in range(8):
            q.cnot(i, i + 1)
        return q

    bare = circuit(qa.create_simulator(9, precision=prec, layers=["cpu"], seed=3))
    q = circuit(qa.create_simulator(9, precision=prec, layers=layers, seed=3))
    for kept in ([8, 0, 4], [2]):
        want = bare.reduced_density_matrix(kept)
        assert np.abs(q.reduced_density_matrix(kept) - want).max() <= STATE_TOL[prec]
    one = np.asarray(q.reduced_density_matrix(4))
    assert np.abs(one - np.asarray(bare.reduced_density_matrix(4))).max() <= STATE_TOL[prec]


@pytest.mark.parametrize("prec", PRECS)
def test_generic_lowering(prec):
    q, sv = cpu_with_state(8, prec, 800, layers=["sparse"])
    for kept in ([0], [7, 1], [5, 2, 6, 0], list(range(8))):
        got = q.reduced_density_matrix(kept)
        ro.check(got, ro.rdm(sv, kept), prec, 0, kept)
        assert got.tobytes() == q.reduced_density_matrix(kept).tobytes()


# ---- helpers -------------------------------------------------------------------------


def test_helpers():
    q = qa.create_simulator(3, engine="cpu", seed=1)
    q.h(0)
    q.cnot(0, 1)
    assert abs(qa.entanglement_entropy(q, [0]) - 1.0) <= 1e-6
    assert abs(qa.purity(q, [0]) - 0.5) <= 1e-6
    assert abs(qa.entanglement_entropy(q, [0], base=math.e) - math.log(2.0)) <= 1e-6
    # qubits 0 and 1 together, and qubit 2 alone, are in a pure state
    for kept in ([0, 1], [2]):
        assert abs(qa.entanglement_entropy(q, kept)) <= 1e-6
        assert abs(qa.purity(q, kept) - 1.0) <= 1e-6


# ---- C ABI and pinvoke -----------------------------------------------------------------


def test_c_abi_and_pinvoke_agree_with_python():
    lib = ctypes.CDLL(glob.glob(os.path.join(ROOT, "qrack_amd", "_qrack*.so"))[0])
    u64 = ctypes.c_uint64
    lib.qrack_init_count_type.restype = u64
    lib.init_count.restype = u64
    lib.init_count.argtypes = [u64, ctypes.c_bool, ctypes.c_bool]
    kept = [4, 1]

    def circuit(h, ry, cx):
        for i in range(6):
            ry(0.4 + 0.25 * i, i)
        for i in range(5):
            cx(i, i + 1)
        h(3)

    q = qa.create_simulator(6, engine="cpu", seed=1)
    circuit(q.h, q.ry, q.cnot)
    want = q.reduced_density_matrix(kept)

    # native entry: doubles out
    sid = lib.qrack_init_count_type(6, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert sid != 0
    circuit(
        lambda t: lib.qrack_h(u64(sid), u64(t)),
        lambda a, t: lib.qrack_r(u64(sid), ctypes.c_int(3), ctypes.c_double(a), u64(t)),
        lambda c, t: lib.qrack_mcx(u64(sid), (u64 * 1)(c), u64(1), u64(t)),
    )
    out = (ctypes.c_double * 32)()
    lib.qrack_reduced_density_matrix(u64(sid), (u64 * 2)(*kept), u64(2), out)
    assert lib.qrack_get_error(u64(sid)) == 0
    got = np.array(out).reshape(4, 4, 2)
    assert np.abs(got[..., 0] + 1j * got[..., 1] - want).max() <= 2e-6
    lib.qrack_reduced_density_matrix(u64(sid), (u64 * 2)(1, 1), u64(2), out)
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))

    # pinvoke layer: floats out
    pid = lib.init_count(u64(6), False, False)
    circuit(
        lambda t: lib.H(u64(pid), u64(t)),
        lambda a, t: lib.R(u64(pid), u64(3), ctypes.c_double(a), u64(t)),
        lambda c, t: lib.MCX(u64(pid), u64(1), (u64 * 1)(c), u64(t)),
    )
    outf = (ctypes.c_float * 32)()
    lib.OutReducedDensityMatrix(u64(pid), u64(2), (u64 * 2)(*kept), outf)
    assert lib.get_error(u64(pid)) == 0
    gotf = np.array(outf, dtype=np.float64).reshape(4, 4, 2)
    assert np.abs(gotf[..., 0] + 1j * gotf[..., 1] - want).max() <= 2e-6
    lib.destroy(u64(pid))


# ---- example ---------------------------------------------------------------------------


def test_example_runs_on_the_cpu_engine():
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "entanglement_growth.py"), "--engine", "cpu"],
        capture_output=True, text=True, timeout=120,
        env={**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")},
    )
    assert r.returncode == 0, r.stderr
    s = [float(line.split()[-1]) for line in r.stdout.splitlines() if line.startswith("t=")]
    assert len(s) >= 5 and s[0] == 0.0
    assert all(b >= a for a, b in zip(s[:5], s[1:5])) and s[4] > 0.01
