"""Plain numpy oracle for the gate path: every gate the engines expose, in
complex128, written from the documented conventions and importing nothing
from qrack_amd.

Conventions
- Bit q of the amplitude index is qubit q.
- A 2x2 is row-major [m00, m01, m10, m11] over (target clear, target set).
- Controls / anti-controls select the subspace where every control is set /
  clear; the rest of the state is untouched.
- mtrx_2q(m, q1, q2) is row-major over the basis index 2*bit(q2) + bit(q1),
  whichever of q1 and q2 is the larger qubit.
- fsim(theta, phi, q1, q2) mixes |01> and |10> by [[cos, -i sin],
  [-i sin, cos]]; |11> gains e^{-i phi}.
- cphase_pairs multiplies by e^{+i angle} where control and target are both
  set; pairs may share qubits and the angles add.
- phase_parity(r, mask) multiplies odd parity of (index & mask) by
  e^{+i r/2} and even parity by e^{-i r/2}; a zero mask is a no-op (the
  engines return before touching the state).
- uniformly_controlled_single_bit(controls, t, ms) applies ms[sel], where
  bit b of sel is the value of controls[b] (list order, not sorted order).
- Batches apply in list order (this matters only for the non-disjoint
  fallbacks; disjoint gates commute).

Every step also updates a companion vector `a`: it starts as |v| and goes
through the same index pattern with |M| in place of M, so a_i bounds the
magnitude of every partial sum that forms amplitude i. `gates` counts the
matrices applied. gate_cases.check_result writes its tolerance in terms of
both.
"""

import numpy as np


def random_state(n, rng):
    """Normalised complex Gaussian state: every amplitude distinct, non-zero."""
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return v / np.linalg.norm(v)


class State:
    def __init__(self, v):
        self.v = np.array(v, dtype=np.complex128)
        self.a = np.abs(self.v)
        self.n = int(self.v.size).bit_length() - 1
        assert self.v.size == 1 << self.n
        self.gates = 0

    # ---- the one primitive -------------------------------------------------
    def apply(self, qubits, m, controls=(), anti=False):
        """The 2^k x 2^k matrix m over `qubits` (bit g of the row / column
        index is qubits[g]) on the subspace selected by `controls`."""
        qubits = list(qubits)
        k = len(qubits)
        m = np.asarray(m, dtype=np.complex128).reshape(1 << k, 1 << k)
        assert len(set(qubits) | set(controls)) == k + len(controls)
        idx = np.arange(self.v.size)
        tmask = sum(1 << q for q in qubits)
        cmask = sum(1 << c for c in controls)
        base = idx[((idx & tmask) == 0) & ((idx & cmask) == (0 if anti else cmask))]
        offs = [sum(1 << qubits[g] for g in range(k) if s >> g & 1) for s in range(1 << k)]
        rows = np.stack([base | o for o in offs])
        self.v[rows] = m @ self.v[rows]
        self.a[rows] = np.abs(m) @ self.a[rows]
        self.gates += 1

    # ---- single-qubit gates and their controlled forms ----------------------
    def mtrx(self, m, t):
        self.apply([t], m)

    def phase(self, tl, br, t):
        self.apply([t], [tl, 0, 0, br])

    def invert(self, tr, bl, t):
        self.apply([t], [0, tr, bl, 0])

    def mcmtrx(self, c, m, t):
        self.apply([t], m, c)

    def macmtrx(self, c, m, t):
        self.apply([t], m, c, anti=True)

    def mcphase(self, c, tl, br, t):
        self.apply([t], [tl, 0, 0, br], c)

    def macphase(self, c, tl, br, t):
        self.apply([t], [tl, 0, 0, br], c, anti=True)

    def mcinvert(self, c, tr, bl, t):
        self.apply([t], [0, tr, bl, 0], c)

    def macinvert(self, c, tr, bl, t):
        self.apply([t], [0, tr, bl, 0], c, anti=True)

    def x(self, t):
        self.invert(1, 1, t)

    def y(self, t):
        self.invert(-1j, 1j, t)

    def z(self, t):
        self.phase(1, -1, t)

    def cnot(self, c, t):
        self.mcinvert([c], 1, 1, t)

    def anti_cnot(self, c, t):
        self.macinvert([c], 1, 1, t)

    def ccnot(self, c1, c2, t):
        self.mcinvert([c1, c2], 1, 1, t)

    def cz(self, c, t):
        self.mcphase([c], 1, -1, t)

    # ---- two-qubit gates ---------------------------------------------------
    def _mid(self, block, q1, q2, controls=()):
        """A 2x2 block on (|01>, |10>) of (q1, q2); |00> and |11> fixed."""
        m = np.eye(4, dtype=np.complex128)
        m[1:3, 1:3] = np.asarray(block, dtype=np.complex128).reshape(2, 2)
        self.apply([q1, q2], m, controls)

    def swap(self, q1, q2):
        self._mid([0, 1, 1, 0], q1, q2)

    def iswap(self, q1, q2):
        self._mid([0, 1j, 1j, 0], q1, q2)

    def sqrt_swap(self, q1, q2):
        self._mid([0.5 + 0.5j, 0.5 - 0.5j, 0.5 - 0.5j, 0.5 + 0.5j], q1, q2)

    def cswap(self, c, q1, q2):
        self._mid([0, 1, 1, 0], q1, q2, c)

    def csqrt_swap(self, c, q1, q2):
        self._mid([0.5 + 0.5j, 0.5 - 0.5j, 0.5 - 0.5j, 0.5 + 0.5j], q1, q2, c)

    def fsim(self, theta, phi, q1, q2):
        c, s = np.cos(theta), np.sin(theta)
        m = np.eye(4, dtype=np.complex128)
        m[1:3, 1:3] = [[c, -1j * s], [-1j * s, c]]
        m[3, 3] = np.exp(-1j * phi)
        self.apply([q1, q2], m)

    def mtrx_2q(self, m, q1, q2):
        self.apply([q1, q2], m)

    # ---- batches -----------------------------------------------------------
    def mtrx_1q_batch(self, targets, ms):
        ms = np.asarray(ms, dtype=np.complex128).reshape(-1, 4)
        for t, m in zip(targets, ms):
            self.mtrx(m, t)

    def mtrx_2q_batch(self, ms, q1s, q2s):
        ms = np.asarray(ms, dtype=np.complex128).reshape(-1, 16)
        for m, q1, q2 in zip(ms, q1s, q2s):
            self.mtrx_2q(m, q1, q2)

    def fsim_batch(self, thetas, phis, q1s, q2s):
        for th, ph, q1, q2 in zip(thetas, phis, q1s, q2s):
            self.fsim(th, ph, q1, q2)

    def cphase_pairs(self, controls, targets, angles):
        for c, t, ang in zip(controls, targets, angles):
            self.mcphase([c], 1, np.exp(1j * ang), t)

    def cz_batch(self, controls, targets):
        for c, t in zip(controls, targets):
            self.cz(c, t)

    def cnot_batch(self, controls, targets):
        for c, t in zip(controls, targets):
            self.cnot(c, t)

    # ---- mask gates --------------------------------------------------------
    def _bits(self, mask):
        return [q for q in range(self.n) if mask >> q & 1]

    def x_mask(self, mask):
        for q in self._bits(mask):
            self.x(q)

    def y_mask(self, mask):
        for q in self._bits(mask):
            self.y(q)

    def z_mask(self, mask):
        for q in self._bits(mask):
            self.z(q)

    def phase_parity(self, r, mask):
        if not mask:
            return
        idx = np.arange(self.v.size)
        odd = np.zeros(self.v.size, dtype=bool)
        for q in self._bits(mask):
            odd ^= (idx >> q & 1).astype(bool)
        self.v *= np.where(odd, np.exp(0.5j * r), np.exp(-0.5j * r))
        self.gates += 1

    # ---- multiplexer -------------------------------------------------------
    def uniformly_controlled_single_bit(self, controls, t, ms):
        ms = np.asarray(ms, dtype=np.complex128).reshape(-1, 2, 2)
        assert ms.shape[0] == 1 << len(controls) and t not in controls
        idx = np.arange(self.v.size)
        base = idx[(idx >> t & 1) == 0]
        sel = np.zeros(base.size, dtype=np.int64)
        for b, c in enumerate(controls):
            sel |= (base >> c & 1) << b
        m = ms[sel]
        x, y = self.v[base], self.v[base | 1 << t]
        ax, ay = self.a[base], self.a[base | 1 << t]
        self.v[base] = m[:, 0, 0] * x + m[:, 0, 1] * y
        self.v[base | 1 << t] = m[:, 1, 0] * x + m[:, 1, 1] * y
        am = np.abs(m)
        self.a[base] = am[:, 0, 0] * ax + am[:, 0, 1] * ay
        self.a[base | 1 << t] = am[:, 1, 0] * ax + am[:, 1, 1] * ay
        self.gates += 1
