"""Plain numpy oracle for the QFT family: the transform column by column
from its definition, the ramp primitives the pagers build theirs from, and
the closed DFT form to hold the columns to. Imports nothing from qrack_amd.

Conventions
- Bit q of the amplitude index is qubit q. No terminal swaps: the output
  register is bit-reversed.
- Forward QFT over bits start..start+length-1: for i = length-1 .. 0, H on
  bit start+i, then every amplitude whose bit start+i is set is multiplied
  by exp(i pi ((x >> start) mod 2^i) / 2^i): the whole ladder of controlled
  phases of column i (control j contributes pi 2^j / 2^i).
- Inverse: the same columns for i = 0 .. length-1, ramp first, then H, with
  the angles negated.
- phase_ramp: amp *= exp(i scale ((x >> ramp_start) mod 2^ramp_bits)) where
  cond_pow == 0 or (x & cond_pow).
- phase_ramp_general: frac(x) = ((x >> ramp_start) & in_place_mask)
  + sum_k bit(x, pows[k]) weights[k]; amp *= exp(i scale frac) on the
  cond_pow half (everywhere if 0).
- qft_column_general: H on `target` and exp(i (scale frac + phase0)) on the
  target-set half; pre=True applies the ramp before the H.

Precision: the work dtype is the dtype of the array passed in.
np.clongdouble (with a long-double pi and long-double sin / cos) wherever
the caller can afford it, np.complex128 for the widest fp32 cases. LONG_OK
says whether the long double of this machine is wide enough to referee
fp64 (eps < 2^-60: the x87 80-bit format has 2^-63).
"""

import numpy as np

LONG_EPS = float(np.finfo(np.longdouble).eps)
LONG_OK = LONG_EPS < 2.0**-60
_LD_PI = np.longdouble("3.14159265358979323846264338327950288")


def work(v, long=True):
    """A fresh work copy of v in the oracle's dtype."""
    return np.array(v, dtype=np.clongdouble if long else np.complex128)


def _real(v):
    return np.longdouble if v.dtype == np.clongdouble else np.float64


def pi_of(v):
    return _LD_PI if v.dtype == np.clongdouble else np.float64(np.pi)


def _cis(theta):
    return np.cos(theta) + 1j * np.sin(theta)


def _n_of(v):
    n = int(v.size).bit_length() - 1
    assert v.size == 1 << n
    return n


def h(v, t):
    """Hadamard on bit t, in place."""
    s = 1 / np.sqrt(_real(v)(2))
    w = v.reshape(-1, 2, 1 << t)
    a = w[:, 0, :].copy()
    b = w[:, 1, :].copy()
    w[:, 0, :] = (a + b) * s
    w[:, 1, :] = (a - b) * s


def _ladder(v, start, i, sign, drop_ctrl=None):
    """Column i's ladder: exp(sign i pi frac / 2^i) on the bit start+i half,
    frac = (x >> start) mod 2^i, without control `drop_ctrl` if given."""
    if not i:
        return
    real = _real(v)
    k = np.arange(1 << i, dtype=np.int64)
    if drop_ctrl is not None:
        k = k & ~np.int64(1 << drop_ctrl)
    table = _cis(real(sign) * pi_of(v) * k.astype(real) / real(1 << i))
    # index layout [above | bit start+i | frac (i bits) | below (start bits)]
    w = v.reshape(-1, 2, 1 << i, 1 << start)
    w[:, 1, :, :] *= table[None, :, None]


def qft(v, start, length, inverse=False, drop=None):
    """QFT / IQFT of bits start..start+length-1 of v, in place and returned.
    drop=(col, ctrl) leaves out the one controlled phase of column `col`
    whose control is bit start+ctrl."""
    assert start + length <= _n_of(v)
    cols = range(length) if inverse else range(length - 1, -1, -1)
    for i in cols:
        dc = drop[1] if drop is not None and drop[0] == i else None
        assert dc is None or dc < i
        if inverse:
            _ladder(v, start, i, -1, dc)
            h(v, start + i)
        else:
            h(v, start + i)
            _ladder(v, start, i, +1, dc)
    return v


def qftr(v, qubits, inverse=False):
    """The same columns over an arbitrary qubit list: column i is H on
    qubits[i] and a phase pi 2^j / 2^i controlled by qubits[j], j < i."""
    real = _real(v)
    idx = np.arange(v.size, dtype=np.int64)
    cols = range(len(qubits)) if inverse else range(len(qubits) - 1, -1, -1)
    for i in cols:
        frac = np.zeros(v.size, dtype=np.int64)
        for j in range(i):
            frac += ((idx >> qubits[j]) & 1) << j
        sel = (idx >> qubits[i]) & 1 == 1
        sign = -1 if inverse else 1
        f = _cis(real(sign) * pi_of(v) * frac[sel].astype(real) / real(1 << i))
        if inverse:
            v[sel] *= f
            h(v, qubits[i])
        else:
            h(v, qubits[i])
            v[sel] *= f
    return v


def _frac_general(v, ramp_start, in_place_mask, pows, weights):
    idx = np.arange(v.size, dtype=np.int64)
    frac = (idx >> ramp_start) & np.int64(in_place_mask)
    for p, w in zip(pows, weights):
        frac = frac + np.where(idx & np.int64(p), np.int64(w), np.int64(0))
    return idx, frac


def _apply_phase(v, idx, frac, scale, phase0, cond_pow):
    real = _real(v)
    theta = real(scale) * frac.astype(real) + real(phase0)
    f = _cis(theta)
    if cond_pow:
        sel = (idx & np.int64(cond_pow)) != 0
        v[sel] *= f[sel]
    else:
        v *= f


def phase_ramp(v, scale, ramp_start, ramp_bits, cond_pow):
    idx = np.arange(v.size, dtype=np.int64)
    frac = (idx >> ramp_start) & np.int64((1 << ramp_bits) - 1)
    _apply_phase(v, idx, frac, scale, 0, cond_pow)
    return v


def phase_ramp_general(v, scale, ramp_start, in_place_mask, pows, weights, cond_pow):
    idx, frac = _frac_general(v, ramp_start, in_place_mask, pows, weights)
    _apply_phase(v, idx, frac, scale, 0, cond_pow)
    return v


def qft_column_general(v, target, scale, ramp_start, in_place_mask, pows, weights,
                       phase0=0.0, pre=False):
    idx, frac = _frac_general(v, ramp_start, in_place_mask, pows, weights)
    if pre:
        _apply_phase(v, idx, frac, scale, phase0, 1 << target)
        h(v, target)
    else:
        h(v, target)
        _apply_phase(v, idx, frac, scale, phase0, 1 << target)
    return v


def bit_reverse(x, n):
    x = np.asarray(x, dtype=np.int64)
    r = np.zeros_like(x)
    for b in range(n):
        r |= ((x >> b) & 1) << (n - 1 - b)
    return r


def dft_bitrev(v, n):
    """The start-0 full-width forward transform in closed form (complex128):
    out[bitrev(k)] = sum_x v[x] exp(2 pi i x k / N) / sqrt(N)."""
    v = np.asarray(v, dtype=np.complex128)
    assert v.size == 1 << n
    spec = np.fft.ifft(v) * np.sqrt(float(v.size))
    out = np.empty_like(spec)
    out[bit_reverse(np.arange(v.size), n)] = spec
    return out
