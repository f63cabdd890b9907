"""qrack_lanczos_lowest_states: the C ABI returns the Python call's values bit
for bit on an fp64 CPU-engine simulator holding the same state.
"""
import ctypes

import numpy as np

import eigen_cases as ec
import krylov_cases as kc
import test_krylov_capi as base

u64 = ctypes.c_uint64
dbl, cint = ctypes.c_double, ctypes.c_int
N = base.N


def _call(lib, sid, terms, nev, dim, tol, max_restarts, prepare):
    lib.qrack_lanczos_lowest_states.restype = u64
    values, residuals = (dbl * nev)(), (dbl * nev)()
    hv, hr = (dbl * ((max_restarts + 1) * nev))(), (dbl * ((max_restarts + 1) * nev))()
    conv, restarts, applies = cint(), cint(), cint()
    m = lib.qrack_lanczos_lowest_states(
        u64(sid), *base._flat(terms), cint(nev), cint(dim), dbl(tol), cint(max_restarts), cint(prepare),
        values, residuals, ctypes.byref(conv), ctypes.byref(restarts), ctypes.byref(applies), hv, hr)
    rows = restarts.value + 1
    info = {"converged": bool(conv.value), "restarts": restarts.value, "applies": applies.value,
            "history_values": np.array(hv[:rows * nev]).reshape(rows, nev),
            "history_residuals": np.array(hr[:rows * nev]).reshape(rows, nev)}
    return np.array(values[:m]), np.array(residuals[:m]), info


def test_c_abi_reproduces_python_bit_for_bit():
    lib = base._lib()
    terms = kc.chain_terms(N)
    sid = base._prepared(lib, 1)
    psi = base._amplitudes(lib, sid)
    twin = base._python_twin(psi)

    got = _call(lib, sid, terms, 2, 6, 0.0, 3, -1)
    assert lib.qrack_get_error(u64(sid)) == 0
    want = ec.call(twin, terms, 2, 6, 0.0, 3, -1)
    assert want[2]["restarts"] == 3 and len(want[0]) == 2
    assert ec.blob(*got) == ec.blob(*want)
    assert np.array_equal(base._amplitudes(lib, sid), psi)

    # a tolerance that ends the run early, and a prepared vector
    got = _call(lib, sid, terms, 2, 8, 1e-3, 16, 1)
    want = ec.call(twin, terms, 2, 8, 1e-3, 16, 1)
    assert want[2]["converged"] and ec.blob(*got) == ec.blob(*want)
    assert np.array_equal(base._amplitudes(lib, sid), np.asarray(twin.get_state_vector()).astype(np.complex128))

    # NULL histories are allowed
    lib.qrack_lanczos_lowest_states.restype = u64
    values, residuals = (dbl * 2)(), (dbl * 2)()
    conv, restarts, applies = cint(), cint(), cint()
    m = lib.qrack_lanczos_lowest_states(
        u64(sid), *base._flat(terms), cint(2), cint(6), dbl(0.0), cint(1), cint(-1), values, residuals,
        ctypes.byref(conv), ctypes.byref(restarts), ctypes.byref(applies), None, None)
    assert m == 2 and restarts.value == 1 and lib.qrack_get_error(u64(sid)) == 0

    # errors land on the handle
    assert len(_call(lib, sid, terms, 2, 3, 0.0, 3, -1)[0]) == 0
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))
