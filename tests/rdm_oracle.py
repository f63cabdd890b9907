"""Independent oracle for reduced density matrices: plain numpy in float64 on
a state vector the engine hands out, so that gate rounding stays out of it.

rho[a, b] = sum_e psi[e, a] conj(psi[e, b]); bit j of a row or column index is
the value of qubits[j] (the order given is honoured).

Tolerance (derived, not measured). Each product carries a few ulp of the real
type R; a run of E_R terms summed in R adds at most E_R ulp of sum|terms|;
Cauchy-Schwarz bounds sum_e |psi[e,a]||psi[e,b]| by sqrt(rho_aa rho_bb). Hence

    |got - want|[a, b] <= (4 + E_R) eps_R sqrt(want_aa want_bb) + 1e-300

with E_R the longest in-R summation run of the implementation: 0 on the CPU
engine and in the generic lowering, qa.RDM_RUN on the HIP engine.
"""
import numpy as np

EPS = {"fp32": float(np.finfo(np.float32).eps), "fp64": float(np.finfo(np.float64).eps)}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}


def random_state(n, rng, dtype):
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    v /= np.linalg.norm(v)
    return v.astype(dtype)


def rdm(sv, qubits):
    """Reduced density matrix of `qubits` of the state vector sv, float64."""
    sv = np.asarray(sv).astype(np.complex128)
    n = int(sv.size).bit_length() - 1
    k = len(qubits)
    t = sv.reshape((2,) * n)  # axis i is qubit n-1-i
    kept_axes = [n - 1 - q for q in qubits]
    env_axes = [ax for ax in range(n) if ax not in kept_axes]
    # kept axes last, qubits[k-1] first among them: qubits[0] is the lowest bit
    t = np.transpose(t, env_axes + kept_axes[::-1])
    A = t.reshape(1 << (n - k), 1 << k)
    return np.einsum("ea,eb->ab", A, A.conj())


def bound(want, prec, e_r):
    d = np.sqrt(np.abs(want.diagonal().real))
    return (4 + e_r) * EPS[prec] * np.outer(d, d) + 1e-300


def check(got, want, prec, e_r, what=None):
    """Shape, dtype, exact Hermiticity, zero diagonal imaginary parts, bound."""
    got = np.asarray(got)
    assert got.dtype == np.complex128 and got.shape == want.shape, what
    assert np.array_equal(got, got.conj().T), what
    assert np.all(got.diagonal().imag == 0.0), what
    err = np.abs(got - want)
    lim = bound(want, prec, e_r)
    assert np.all(err <= lim), (what, float((err / lim).max()))
