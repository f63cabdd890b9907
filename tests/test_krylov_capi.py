"""qrack_lanczos_tridiagonal, qrack_krylov_evolve_pauli_sum and
qrack_lanczos_ground_state: the C ABI reproduces the Python calls on an fp64
CPU-engine simulator holding the same state.
"""
import ctypes
import glob
import os

import numpy as np

import qrack_amd as qa
import krylov_cases as kc
import krylov_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = ctypes.c_uint64
N = 5


def _flat(terms):
    coeffs = (ctypes.c_double * len(terms))(*[c for c, _, _ in terms])
    lens = (u64 * len(terms))(*[len(qs) for _, qs, _ in terms])
    qs = [q for _, qs_, _ in terms for q in qs_]
    ps = [p for _, _, ps_ in terms for p in ps_]
    return (u64(len(terms)), coeffs, lens, (u64 * max(1, len(qs)))(*qs), (ctypes.c_int * max(1, len(ps)))(*ps))


def _lib():
    lib = ctypes.CDLL(glob.glob(os.path.join(ROOT, "qrack_amd", "_qrack*.so"))[0])
    lib.qrack_init_count_type.restype = u64
    lib.qrack_lanczos_tridiagonal.restype = u64
    lib.qrack_krylov_evolve_pauli_sum.restype = ctypes.c_double
    lib.qrack_lanczos_ground_state.restype = ctypes.c_double
    return lib


def _prepared(lib, seed):
    """a 5-qubit fp64 CPU-engine state built with gates"""
    sid = lib.qrack_init_count_type(u64(N), 0, 0, 0, 0, 0, 0, 0, 0, 1)
    assert sid != 0
    r = np.random.default_rng(seed)
    for q in range(N):
        lib.qrack_u(u64(sid), u64(q), ctypes.c_double(r.uniform(0, 3)),
                    ctypes.c_double(r.uniform(0, 3)), ctypes.c_double(r.uniform(0, 3)))
    for q in range(N - 1):
        lib.qrack_mcx(u64(sid), (u64 * 1)(q), u64(1), u64(q + 1))
    return sid


def _amplitudes(lib, sid):
    out = np.zeros(1 << N, dtype=np.complex128)
    re, im = ctypes.c_double(), ctypes.c_double()
    for i in range(1 << N):
        lib.qrack_get_amplitude(u64(sid), u64(i), ctypes.byref(re), ctypes.byref(im))
        out[i] = complex(re.value, im.value)
    return out


def _python_twin(psi):
    q = qa.create_simulator(N, engine="cpu", precision="fp64", seed=1)
    q.set_state_vector(psi)
    return q


def test_c_abi_reproduces_python():
    lib = _lib()
    terms = kc.chain_terms(N)
    s = ko.sum_abs(terms)
    dbl, cint = ctypes.c_double, ctypes.c_int
    sid = _prepared(lib, 1)
    psi = _amplitudes(lib, sid)
    twin = _python_twin(psi)

    dim = 6
    alpha, beta = (dbl * dim)(), (dbl * dim)()
    k = lib.qrack_lanczos_tridiagonal(u64(sid), *_flat(terms), cint(dim), alpha, beta)
    assert lib.qrack_get_error(u64(sid)) == 0
    wa, wb = twin.lanczos_tridiagonal(terms, dim)
    assert k == len(wa) == dim
    assert np.abs(np.array(alpha[:k]) - wa).max() <= 1e-12 * s
    assert np.abs(np.array(beta[:k]) - wb).max() <= 1e-12 * s
    assert np.array_equal(_amplitudes(lib, sid), psi)

    res = dbl()
    e = lib.qrack_lanczos_ground_state(u64(sid), *_flat(terms), cint(dim), cint(0), ctypes.byref(res))
    we, wres = twin.lanczos_ground_state(terms, dim, False)
    assert abs(e - we) <= 1e-12 * s and abs(res.value - wres) <= 1e-12 * s
    assert np.array_equal(_amplitudes(lib, sid), psi)

    est = lib.qrack_krylov_evolve_pauli_sum(u64(sid), *_flat(terms), dbl(0.3), cint(dim), cint(2))
    assert lib.qrack_get_error(u64(sid)) == 0
    west = twin.krylov_evolve_pauli_sum(terms, 0.3, dim, 2)
    assert abs(est - west) <= 1e-12 * s
    assert np.abs(_amplitudes(lib, sid) - np.asarray(twin.get_state_vector())).max() <= 1e-12

    e = lib.qrack_lanczos_ground_state(u64(sid), *_flat(terms), cint(dim), cint(1), ctypes.byref(res))
    we, wres = twin.lanczos_ground_state(terms, dim, True)
    assert abs(e - we) <= 1e-12 * s and abs(res.value - wres) <= 1e-12 * s
    assert kc.phase_distance(_amplitudes(lib, sid), np.asarray(twin.get_state_vector()).astype(np.complex128)) <= 1e-12

    # errors land on the handle: dim 0, steps 0, a bad Pauli code
    assert lib.qrack_lanczos_tridiagonal(u64(sid), *_flat(terms), cint(0), alpha, beta) == 0
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))
    sid = _prepared(lib, 2)
    assert lib.qrack_krylov_evolve_pauli_sum(u64(sid), *_flat(terms), dbl(0.3), cint(dim), cint(0)) == 0.0
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))
    sid = _prepared(lib, 3)
    lib.qrack_lanczos_ground_state(u64(sid), *_flat([(1.0, [0], [7])]), cint(dim), cint(0), ctypes.byref(res))
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))
