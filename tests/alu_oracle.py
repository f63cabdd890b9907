"""Plain numpy oracle for the permutation ALU, the structural operations and
the reductions. It holds no engine code: every function builds its answer
from `np.arange(1 << n)` with shifts, masks and one fancy-index scatter.

Conventions: qubit 0 is the low bit of the state index; a state is a
complex128 vector of length 2^n; every ALU function has the signature of
the Python method of the same name, with the state in front, and returns a
new state.

Preconditions are checked, not assumed: an op that is a permutation only on
part of the space (carry/out register in |0>, a definite carry qubit, a
dividend that is a multiple of the divisor) asserts that the input has no
amplitude outside that part.
"""

import numpy as np

_FULL = (1 << 64) - 1


def _idx(state):
    n = int(state.size).bit_length() - 1
    assert state.size == 1 << n
    return np.arange(1 << n, dtype=np.uint64)


def _lowmask(length):
    return np.uint64((1 << length) - 1)


def _field(idx, start, length):
    return (idx >> np.uint64(start)) & _lowmask(length)


def _put(idx, start, length, value):
    keep = np.uint64(_FULL ^ (((1 << length) - 1) << start))
    return (idx & keep) | ((value & _lowmask(length)) << np.uint64(start))


def _all_set(idx, bits):
    mask = np.uint64(sum(1 << b for b in bits))
    return (idx & mask) == mask


def _scatter(state, dest, sel=None, keep=None):
    """out[dest[i]] = state[i] for i in `sel`; out[i] = state[i] for i in
    `keep`; every other input slot must be empty and no slot is hit twice."""
    n_amp = state.size
    sel = np.ones(n_amp, dtype=bool) if sel is None else sel
    keep = np.zeros(n_amp, dtype=bool) if keep is None else keep
    assert not np.any(sel & keep)
    assert not np.any(state[~(sel | keep)]), "input violates the op's precondition"
    out = np.zeros_like(state)
    out[keep] = state[keep]
    d = dest[sel]
    hits = np.bincount(d.astype(np.int64), minlength=n_amp) + keep
    assert hits.max() <= 1, "oracle map is not injective"
    out[d] = state[sel]
    return out


def _table(values, entries, length):
    """Little-endian entries of ceil(length/8) bytes each, masked to length."""
    nbytes = (length + 7) // 8
    raw = np.frombuffer(bytes(values), dtype=np.uint8)[: entries * nbytes]
    raw = raw.reshape(entries, nbytes).astype(np.uint64)
    out = np.zeros(entries, dtype=np.uint64)
    for b in range(nbytes):
        out |= raw[:, b] << np.uint64(8 * b)
    return out & _lowmask(length)


def _definite_bit(state, idx, bit):
    """Value of a qubit that the input holds in a basis state."""
    one = ((idx >> np.uint64(bit)) & np.uint64(1)) == 1
    has1, has0 = bool(np.any(state[one])), bool(np.any(state[~one]))
    assert not (has0 and has1), "carry qubit must be in a basis state"
    return (1 if has1 else 0), one


# ---- state helpers -----------------------------------------------------------


def random_state(n, rng, zero_mask=0):
    """Normalised complex Gaussian state with no amplitude where
    (index & zero_mask) != 0."""
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    idx = np.arange(1 << n, dtype=np.uint64)
    v[(idx & np.uint64(zero_mask)) != 0] = 0
    return v / np.linalg.norm(v)


def random_dense_state(n, rng):
    """Normalised state whose magnitudes stay within a factor 3 of each
    other, so no amplitude comes near the engines' amplitude floor
    (|amp|^2 < eps_R is dropped by NormalizeState)."""
    r = rng.uniform(0.5, 1.5, 1 << n)
    v = r * np.exp(1j * rng.uniform(0, 2 * np.pi, 1 << n))
    return v / np.linalg.norm(v)


def x_mask(state, mask):
    """Pauli X on every qubit of `mask`."""
    idx = _idx(state)
    return _scatter(state, idx ^ np.uint64(mask))


# ---- add / subtract ------------------------------------------------------------


def inc(state, to_add, start, length):
    idx = _idx(state)
    reg = _field(idx, start, length)
    return _scatter(state, _put(idx, start, length, reg + np.uint64(to_add % (1 << length))))


def dec(state, to_sub, start, length):
    return inc(state, (1 << length) - (to_sub % (1 << length)), start, length)


def cinc(state, to_add, start, length, controls):
    idx = _idx(state)
    sel = _all_set(idx, controls)
    reg = _field(idx, start, length)
    dest = _put(idx, start, length, reg + np.uint64(to_add % (1 << length)))
    return _scatter(state, dest, sel, ~sel)


def _add_with_carry(state, addend, start, length, carry_index, idx, carry_one):
    """reg += addend on the carry-clear half; carry-out sets the carry."""
    total = _field(idx, start, length) + np.uint64(addend)
    dest = _put(idx, start, length, total)
    dest = dest | (((total >> np.uint64(length)) & np.uint64(1)) << np.uint64(carry_index))
    return _scatter(state, dest, ~carry_one)


def incc(state, to_add, start, length, carry_index):
    """Add with carry. A set carry qubit is consumed as a carry-in of one;
    the addend wraps to the register length before it is added."""
    idx = _idx(state)
    c_in, one = _definite_bit(state, idx, carry_index)
    if c_in:
        state = x_mask(state, 1 << carry_index)
    return _add_with_carry(state, (to_add + c_in) % (1 << length), start, length, carry_index, idx, one)


def decc(state, to_sub, start, length, carry_index):
    """Subtract with borrow: reg - to_sub - (1 - carry_in); the carry ends
    set when no borrow occurred. Requires 0 < to_sub < 2^length."""
    assert 0 < to_sub < (1 << length)
    idx = _idx(state)
    c_in, one = _definite_bit(state, idx, carry_index)
    if c_in:
        state = x_mask(state, 1 << carry_index)
    reg = _field(idx, start, length).astype(np.int64)
    diff = reg - to_sub - (1 - c_in)
    dest = _put(idx, start, length, (diff % (1 << length)).astype(np.uint64))
    dest = dest | ((diff >= 0).astype(np.uint64) << np.uint64(carry_index))
    return _scatter(state, dest, ~one)


def incs(state, to_add, start, length, overflow_index):
    """Signed add: the overflow qubit flips when the two's-complement sum
    leaves [-2^(length-1), 2^(length-1))."""
    idx = _idx(state)
    half = 1 << (length - 1)
    to_add %= 1 << length
    reg = _field(idx, start, length).astype(np.int64)
    s_reg = np.where(reg >= half, reg - 2 * half, reg)
    s_add = to_add - 2 * half if to_add >= half else to_add
    total = s_reg + s_add
    ovf = (total >= half) | (total < -half)
    dest = _put(idx, start, length, (total % (2 * half)).astype(np.uint64))
    dest = dest ^ (ovf.astype(np.uint64) << np.uint64(overflow_index))
    return _scatter(state, dest)


def _bcd_decode(reg, digits):
    value = np.zeros(reg.shape, dtype=np.uint64)
    valid = np.ones(reg.shape, dtype=bool)
    for d in range(digits):
        digit = (reg >> np.uint64(4 * d)) & np.uint64(15)
        valid &= digit <= 9
        value += digit * np.uint64(10**d)
    return value, valid


def _bcd_encode(value, digits):
    enc = np.zeros(value.shape, dtype=np.uint64)
    for d in range(digits):
        enc |= ((value // np.uint64(10**d)) % np.uint64(10)) << np.uint64(4 * d)
    return enc


def incbcd(state, to_add, start, length):
    """Decimal add on 4-bit digits, modulo 10^digits. A register value with
    any digit code above 9 maps to itself."""
    assert length % 4 == 0
    digits = length // 4
    idx = _idx(state)
    value, valid = _bcd_decode(_field(idx, start, length), digits)
    total = (value + np.uint64(to_add % 10**digits)) % np.uint64(10**digits)
    dest = _put(idx, start, length, _bcd_encode(total, digits))
    return _scatter(state, dest, valid, ~valid)


def decbcd(state, to_sub, start, length):
    digits = length // 4
    return incbcd(state, 10**digits - (to_sub % 10**digits), start, length)


# ---- multiply / divide -----------------------------------------------------------


def _controlled(idx, controls):
    if not controls:
        return np.ones(idx.shape, dtype=bool)
    return _all_set(idx, controls)


def cmul(state, to_mul, in_out_start, carry_start, length, controls):
    """(carry:inout) = inout * to_mul on the carry == 0 part of the
    controlled subspace; everything else is untouched."""
    assert 0 < to_mul < (1 << length)
    idx = _idx(state)
    ctl = _controlled(idx, controls)
    sel = ctl & (_field(idx, carry_start, length) == 0)
    prod = _field(idx, in_out_start, length) * np.uint64(to_mul)
    dest = _put(idx, in_out_start, length, prod)
    dest = _put(dest, carry_start, length, prod >> np.uint64(length))
    return _scatter(state, dest, sel, ~ctl)


def cdiv(state, to_div, in_out_start, carry_start, length, controls):
    """Inverse of cmul: (carry:inout) must be to_div * q with q < 2^length,
    and becomes carry = 0, inout = q."""
    assert 0 < to_div < (1 << length)
    idx = _idx(state)
    ctl = _controlled(idx, controls)
    wide = (_field(idx, carry_start, length) << np.uint64(length)) | _field(idx, in_out_start, length)
    quot = wide // np.uint64(to_div)
    sel = ctl & (wide % np.uint64(to_div) == 0) & (quot < (1 << length))
    dest = _put(idx, in_out_start, length, quot)
    dest = _put(dest, carry_start, length, np.zeros_like(quot))
    return _scatter(state, dest, sel, ~ctl)


def mul(state, to_mul, in_out_start, carry_start, length):
    return cmul(state, to_mul, in_out_start, carry_start, length, [])


def div(state, to_div, in_out_start, carry_start, length):
    return cdiv(state, to_div, in_out_start, carry_start, length, [])


def _out_of_in(state, fn, in_start, out_start, length, controls, inverse=False):
    """out = fn(in) from out == 0 (or back to out == 0 when `inverse`)."""
    idx = _idx(state)
    ctl = _controlled(idx, controls)
    lut = np.array([fn(v) for v in range(1 << length)], dtype=np.uint64)
    image = lut[_field(idx, in_start, length).astype(np.int64)]
    out_reg = _field(idx, out_start, length)
    if inverse:
        sel = ctl & (out_reg == image)
        dest = _put(idx, out_start, length, np.zeros_like(image))
    else:
        sel = ctl & (out_reg == 0)
        dest = _put(idx, out_start, length, image)
    return _scatter(state, dest, sel, ~ctl)


def cmul_mod_n_out(state, to_mul, mod_n, in_start, out_start, length, controls):
    assert 0 < mod_n <= (1 << length)
    return _out_of_in(state, lambda v: (v * to_mul) % mod_n, in_start, out_start, length, controls)


def cimul_mod_n_out(state, to_mul, mod_n, in_start, out_start, length, controls):
    assert 0 < mod_n <= (1 << length)
    return _out_of_in(
        state, lambda v: (v * to_mul) % mod_n, in_start, out_start, length, controls, inverse=True
    )


def cpow_mod_n_out(state, base, mod_n, in_start, out_start, length, controls):
    assert 0 < mod_n <= (1 << length)
    return _out_of_in(state, lambda v: pow(base, v, mod_n), in_start, out_start, length, controls)


def mul_mod_n_out(state, to_mul, mod_n, in_start, out_start, length):
    return cmul_mod_n_out(state, to_mul, mod_n, in_start, out_start, length, [])


def imul_mod_n_out(state, to_mul, mod_n, in_start, out_start, length):
    return cimul_mod_n_out(state, to_mul, mod_n, in_start, out_start, length, [])


def pow_mod_n_out(state, base, mod_n, in_start, out_start, length):
    return cpow_mod_n_out(state, base, mod_n, in_start, out_start, length, [])


# ---- table look-ups ----------------------------------------------------------------


def indexed_lda(state, index_start, index_length, value_start, value_length, values, reset_value=True):
    """value = table[index], from value == 0."""
    assert reset_value
    idx = _idx(state)
    table = _table(values, 1 << index_length, value_length)
    loaded = table[_field(idx, index_start, index_length).astype(np.int64)]
    sel = _field(idx, value_start, value_length) == 0
    return _scatter(state, _put(idx, value_start, value_length, loaded), sel)


def indexed_adc(state, index_start, index_length, value_start, value_length, carry_index, values):
    """value += table[index] + carry_in; carry-out sets the carry."""
    idx = _idx(state)
    c_in, one = _definite_bit(state, idx, carry_index)
    if c_in:
        state = x_mask(state, 1 << carry_index)
    table = _table(values, 1 << index_length, value_length)
    total = (
        _field(idx, value_start, value_length)
        + table[_field(idx, index_start, index_length).astype(np.int64)]
        + np.uint64(c_in)
    )
    dest = _put(idx, value_start, value_length, total)
    dest = dest | (((total >> np.uint64(value_length)) & np.uint64(1)) << np.uint64(carry_index))
    return _scatter(state, dest, ~one)


def indexed_sbc(state, index_start, index_length, value_start, value_length, carry_index, values):
    """value -= table[index] + (1 - carry_in); the carry ends set when no
    borrow occurred."""
    idx = _idx(state)
    c_in, one = _definite_bit(state, idx, carry_index)
    if c_in:
        state = x_mask(state, 1 << carry_index)
    table = _table(values, 1 << index_length, value_length).astype(np.int64)
    diff = (
        _field(idx, value_start, value_length).astype(np.int64)
        - table[_field(idx, index_start, index_length).astype(np.int64)]
        - (1 - c_in)
    )
    dest = _put(idx, value_start, value_length, (diff % (1 << value_length)).astype(np.uint64))
    dest = dest | ((diff >= 0).astype(np.uint64) << np.uint64(carry_index))
    return _scatter(state, dest, ~one)


def hash(state, start, length, values):  # noqa: A001 - named after the engine method
    idx = _idx(state)
    table = _table(values, 1 << length, length)
    return _scatter(state, _put(idx, start, length, table[_field(idx, start, length).astype(np.int64)]))


# ---- rotate / phase flip -----------------------------------------------------------


def rol(state, shift, start, length):
    """Bit k of the register moves to bit (k + shift) mod length."""
    idx = _idx(state)
    reg = _field(idx, start, length)
    rot = np.zeros_like(reg)
    for k in range(length):
        rot |= ((reg >> np.uint64(k)) & np.uint64(1)) << np.uint64((k + shift) % length)
    return _scatter(state, _put(idx, start, length, rot))


def ror(state, shift, start, length):
    return rol(state, (length - shift % length) % length, start, length)


def phase_flip_if_less(state, greater_perm, start, length):
    idx = _idx(state)
    out = state.copy()
    out[_field(idx, start, length) < greater_perm] *= -1
    return out


def cphase_flip_if_less(state, greater_perm, start, length, flag_index):
    idx = _idx(state)
    out = state.copy()
    out[(_field(idx, start, length) < greater_perm) & _all_set(idx, [flag_index])] *= -1
    return out


# ---- structural references -----------------------------------------------------------


def _split(idx, start, length):
    """(remainder index, part index) of a full index."""
    low = idx & _lowmask(start)
    high = idx >> np.uint64(start + length)
    return (low | (high << np.uint64(start))).astype(np.int64), _field(idx, start, length).astype(np.int64)


def compose(a, b, start):
    """b's qubits are inserted into a at `start`."""
    n = int(a.size * b.size).bit_length() - 1
    length = int(b.size).bit_length() - 1
    rem, part = _split(np.arange(1 << n, dtype=np.uint64), start, length)
    return a[rem] * b[part]


def allocate(a, start, length):
    zero = np.zeros(1 << length, dtype=a.dtype)
    zero[0] = 1
    return compose(a, zero, start)


def slice_part(state, start, length, perm):
    """Amplitudes of the remainder where the register [start, start+length)
    reads `perm`."""
    rem, part = _split(_idx(state), start, length)
    out = np.zeros(state.size >> length, dtype=state.dtype)
    sel = part == perm
    out[rem[sel]] = state[sel]
    return out


def align_phase(got, expected):
    """`got` times the unit phase that brings it closest to `expected`."""
    inner = np.vdot(expected, got)
    return got * (np.conj(inner) / abs(inner))


# ---- reductions --------------------------------------------------------------------


def probs(state):
    return np.abs(np.asarray(state, dtype=np.complex128)) ** 2


def prob(state, qubit):
    return prob_mask(state, 1 << qubit, 1 << qubit)


def prob_mask(state, mask, perm):
    idx = _idx(state)
    return float(probs(state)[(idx & np.uint64(mask)) == np.uint64(perm)].sum())


def prob_reg(state, start, length, perm):
    return prob_mask(state, ((1 << length) - 1) << start, perm << start)


def _parity(idx, mask):
    m = idx & np.uint64(mask)
    par = np.zeros(idx.shape, dtype=np.uint64)
    while m.any():
        par ^= m & np.uint64(1)
        m = m >> np.uint64(1)
    return par == 1


def prob_parity(state, mask):
    return float(probs(state)[_parity(_idx(state), mask)].sum())


def prob_bits_all(state, bits):
    idx = _idx(state)
    key = np.zeros(idx.shape, dtype=np.int64)
    for k, b in enumerate(bits):
        key |= (((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(k)).astype(np.int64)
    return np.bincount(key, weights=probs(state), minlength=1 << len(bits))


def bit_values(n_amp, bits, perms=None, offset=0):
    """offset + sum over set bits[k] of perms[k] (2^k by default), per index."""
    idx = np.arange(n_amp, dtype=np.uint64)
    perms = [1 << k for k in range(len(bits))] if perms is None else perms
    val = np.full(n_amp, float(offset))
    for b, p in zip(bits, perms):
        val += ((idx >> np.uint64(b)) & np.uint64(1)).astype(np.float64) * float(p)
    return val


def expectation(state, values):
    return float(np.sum(values * probs(state)))


def variance(state, values):
    p = probs(state)
    mean = float(np.sum(values * p))
    return float(np.sum(values * values * p)) - mean * mean


def project(state, keep):
    """Projection onto the indices in the boolean array `keep`, renormalised."""
    out = np.where(keep, state, 0)
    return out / np.linalg.norm(out)


def project_mask(state, mask, perm):
    idx = _idx(state)
    return project(state, (idx & np.uint64(mask)) == np.uint64(perm))


def project_parity(state, mask, odd):
    return project(state, _parity(_idx(state), mask) == bool(odd))


def sum_sqr_diff(a, b):
    """min over phi of sum |a - e^{i phi} b|^2 = 2 - 2 |<b|a>| for unit vectors."""
    return 2.0 - 2.0 * abs(np.vdot(b, a))
