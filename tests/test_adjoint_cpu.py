"""pauli_sum_braket, pauli_sum_apply_into and adjoint_gradient on the CPU
engine, through the wrapping layers, through the generic lowering (QUnit) and
through the C ABI. Oracle and tolerances: adjoint_oracle.py; the checks shared
with the HIP engine's file are in adjoint_cases.py.
"""
import ctypes
import glob
import importlib.util
import os

import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po
import adjoint_oracle as ao
import adjoint_cases as ac

ENGINE = "cpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ac.PRECS


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    ac.widths(ENGINE, n, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("x", ac.x_masks_12(), ids=lambda x: "x%03x" % x)
def test_partner_logic_12(x, prec):
    ac.partner_logic(ENGINE, prec, x)


@pytest.mark.parametrize("prec", PRECS)
def test_conjugation_and_aliasing(prec):
    ac.conjugation_and_aliasing(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_group_larger_than_cap_splits(prec):
    ac.chunking(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_read_only_and_write_all(prec):
    ac.readonly_and_writeall(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_pending_basis_state(prec):
    ac.pending_basis_state(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (5, 9))
def test_gradient(n, prec):
    ac.gradient(ENGINE, n, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_gradient_edges(prec):
    ac.gradient_edges(ENGINE, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layers", (["hybrid"], ["fuser", "cpu"]), ids=lambda l: "-".join(l))
def test_layers_reach_engine(layers, prec):
    ac.layers_match_engine(ENGINE, layers, prec, None)


@pytest.mark.parametrize("prec", PRECS)
def test_qunit_generic_lowering(prec):
    """QUnit keeps the host-copy lowering: oracle values, and its own state
    untouched by all three calls"""
    n = 5
    rng = np.random.default_rng(800)
    terms = po.random_terms(n, rng, 20) + [(0.6, [], [])]
    ops = ac.gradient_circuit(n, rng)
    q, psi = ac.sim_with_state(ENGINE, n, prec, 801, layers=["qunit", "cpu"])
    b, phi = ac.sim_with_state(ENGINE, n, prec, 802, layers=["qunit", "cpu"])
    d, _ = ac.sim_with_state(ENGINE, n, prec, 803, layers=["qunit", "cpu"])
    ac.check_braket(b, phi, q, psi, terms, prec, "qunit")
    ac.check_apply(q, psi, d, terms, prec, "qunit")
    e, g = q.adjoint_gradient(ops, terms)
    want_e, want_g = ao.gradient(psi, ops, terms)
    bound = ao.gradient_bound(ops, terms, prec)
    assert abs(e - want_e) <= bound and np.all(np.abs(g - want_g) <= bound)
    # reading a QUnit's state goes through a clone; compare values, not bytes
    assert np.array_equal(np.asarray(q.get_state_vector()), psi)
    assert np.array_equal(np.asarray(b.get_state_vector()), phi)
    with pytest.raises(Exception):
        q.pauli_sum_apply_into(terms, q)


def test_noise_layer():
    n = 4
    rng = np.random.default_rng(810)
    terms = po.random_terms(n, rng, 8)
    q = qa.create_simulator(n, layers=["noisy", "cpu"], seed=3)
    b = qa.create_simulator(n, layers=["noisy", "cpu"], seed=4)
    d = qa.create_simulator(n, layers=["noisy", "cpu"], seed=5)
    q.set_state_vector(po.random_state(n, rng, np.complex64))
    b.set_state_vector(po.random_state(n, rng, np.complex64))
    psi, phi = np.asarray(q.get_state_vector()), np.asarray(b.get_state_vector())
    with pytest.raises(Exception, match="not defined under gate noise"):
        q.adjoint_gradient([("rot", [0], [1], 0.2)], terms)
    # the two read-style calls are forwarded
    ac.check_braket(b, phi, q, psi, terms, "fp32", "noisy")
    ac.check_apply(q, psi, d, terms, "fp32", "noisy")


# ---- C ABI -----------------------------------------------------------------------


def _flat(terms):
    coeffs = (ctypes.c_double * len(terms))(*[c for c, _, _ in terms])
    lens = (ctypes.c_uint64 * len(terms))(*[len(qs) for _, qs, _ in terms])
    qs = [q for _, qs_, _ in terms for q in qs_]
    ps = [p for _, _, ps_ in terms for p in ps_]
    return (ctypes.c_uint64(len(terms)), coeffs, lens, (ctypes.c_uint64 * max(1, len(qs)))(*qs),
            (ctypes.c_int * max(1, len(ps)))(*ps))


def test_c_abi():
    lib = ctypes.CDLL(glob.glob(os.path.join(ROOT, "qrack_amd", "_qrack*.so"))[0])
    lib.qrack_init_count_type.restype = ctypes.c_uint64
    u64 = ctypes.c_uint64
    n = 5
    rng = np.random.default_rng(820)

    def prepared(seed):
        """a 5-qubit fp64 CPU-engine state built with gates, and its amplitudes"""
        sid = lib.qrack_init_count_type(u64(n), 0, 0, 0, 0, 0, 0, 0, 0, 1)
        assert sid != 0
        r = np.random.default_rng(seed)
        for q in range(n):
            lib.qrack_u(u64(sid), u64(q), ctypes.c_double(r.uniform(0, 3)),
                        ctypes.c_double(r.uniform(0, 3)), ctypes.c_double(r.uniform(0, 3)))
        for q in range(n - 1):
            lib.qrack_mcx(u64(sid), (ctypes.c_uint64 * 1)(q), u64(1), u64(q + 1))
        return sid

    def amplitudes(sid):
        out = np.zeros(1 << n, dtype=np.complex128)
        re, im = ctypes.c_double(), ctypes.c_double()
        for i in range(1 << n):
            lib.qrack_get_amplitude(u64(sid), u64(i), ctypes.byref(re), ctypes.byref(im))
            out[i] = complex(re.value, im.value)
        return out

    ket, bra, dest = prepared(1), prepared(2), prepared(3)
    psi, phi = amplitudes(ket), amplitudes(bra)
    terms = po.random_terms(n, rng, 12) + [(0.5, [], [])]
    re, im = ctypes.c_double(), ctypes.c_double()
    lib.qrack_pauli_sum_braket(u64(ket), u64(bra), *_flat(terms), ctypes.byref(re), ctypes.byref(im))
    assert lib.qrack_get_error(u64(ket)) == 0
    want = ao.braket(phi, psi, terms)
    tol = ao.TOL["fp64"] * po.abs_coeffs(terms)
    assert abs(re.value - want.real) <= tol and abs(im.value - want.imag) <= tol
    lib.qrack_pauli_sum_apply_into(u64(ket), *_flat(terms), u64(dest))
    assert lib.qrack_get_error(u64(ket)) == 0
    hpsi, a = ao.apply_sum(psi, terms)
    assert np.all(np.abs(amplitudes(dest) - hpsi) <= 4 * ao.launches(terms) * ao.EPS["fp64"] * a)
    assert np.array_equal(amplitudes(ket), psi)
    # dest == source is an error, reported on the source handle
    lib.qrack_pauli_sum_apply_into(u64(ket), *_flat(terms), u64(ket))
    assert lib.qrack_get_error(u64(ket)) != 0
    for sid in (ket, bra, dest):
        lib.qrack_destroy(u64(sid))


# ---- example -----------------------------------------------------------------------


def test_vqe_adjoint_example(capsys):
    spec = importlib.util.spec_from_file_location(
        "vqe_adjoint", os.path.join(ROOT, "examples", "vqe_adjoint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    energy, ground, gap = mod.main()
    assert gap == 0.5 * (mod.E_NEEL - ground) and ground < energy < ground + gap
