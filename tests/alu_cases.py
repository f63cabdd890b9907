"""Case table and runner shared by test_alu_oracle_cpu.py and
test_alu_oracle_gpu.py: every ALU op against tests/alu_oracle.py.

A case names an engine method, its arguments, the qubits the input keeps in
|0> (carry / out registers: the documented precondition that makes each op a
unitary permutation) and optional oracle steps that turn the random state
into the op's input (the forward op for an inverse, an X for a set carry).
"""

import zlib
from typing import NamedTuple

import numpy as np

import alu_oracle as ao

EPS = {"fp32": 2.0**-23, "fp64": 2.0**-52}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}


class Case(NamedTuple):
    id: str
    n: int
    op: str
    args: tuple
    zero_mask: int = 0
    pre: tuple = ()
    rescaled: bool = False


def reg(start, length):
    return ((1 << length) - 1) << start


_rng = np.random.default_rng(20241)


def _bytes_table(entries, nbytes):
    return bytes(_rng.integers(0, 256, entries * nbytes, dtype=np.uint8))


def _perm_table(length):
    perm = _rng.permutation(1 << length)
    if length <= 8:
        return bytes(perm.astype(np.uint8))
    return perm.astype("<u2").tobytes()


T8x1 = _bytes_table(8, 1)  # 3 index bits, entries of up to 8 bits
T2x2 = _bytes_table(2, 2)  # 1 index bit, entries of 9..16 bits
T8x2 = _bytes_table(8, 2)
HASH4 = _perm_table(4)
HASH9 = _perm_table(9)


def _carry_pair(name, op, args, carry, n=10):
    """The same call with the carry qubit clear and set on input."""
    return [
        Case(f"{name}-c0", n, op, args, 1 << carry),
        Case(f"{name}-c1", n, op, args, 1 << carry, (("x_mask", (1 << carry,)),), True),
    ]


def _with_inverse(name, fwd, inv, args, zero_mask, n=10):
    """A forward op, and its inverse fed with the forward oracle's output."""
    return [
        Case(name.format(fwd), n, fwd, args, zero_mask),
        Case(name.format(inv), n, inv, args, zero_mask, ((fwd, args),)),
    ]


BASE_CASES = [
    # ---- inc / dec / cinc: start 0, a register across bit 6, the whole width
    Case("inc-s0", 10, "inc", (5, 0, 4)),
    Case("inc-s4", 10, "inc", (11, 4, 4)),
    Case("inc-full", 10, "inc", (777, 0, 10)),
    Case("dec-s0", 10, "dec", (3, 0, 4)),
    Case("dec-s4", 10, "dec", (9, 4, 4)),
    Case("cinc-s0-above", 10, "cinc", (5, 0, 4, [9])),
    Case("cinc-s4-below-above", 10, "cinc", (7, 4, 4, [0, 9])),
    Case("cinc-s3-below", 10, "cinc", (6, 3, 5, [1])),
    # ---- incc / decc: carry above and below the register, clear and set
    *_carry_pair("incc-s0-carry9", "incc", (5, 0, 4, 9), 9),
    *_carry_pair("incc-s4-carry0", "incc", (11, 4, 4, 0), 0),
    *_carry_pair("decc-s0-carry9", "decc", (5, 0, 4, 9), 9),
    *_carry_pair("decc-s4-carry0", "decc", (11, 4, 4, 0), 0),
    # ---- incs: overflow qubit above / below; it is flipped, so it may also be dense
    Case("incs-s0-ovf9", 10, "incs", (5, 0, 4, 9), 1 << 9),
    Case("incs-s4-ovf1", 10, "incs", (11, 4, 4, 1), 1 << 1),
    Case("incs-s4-ovf9-dense", 10, "incs", (3, 4, 4, 9)),
    # ---- BCD: random states hold the non-BCD codes 10..15 too
    Case("incbcd-1digit", 10, "incbcd", (7, 0, 4)),
    Case("incbcd-2digit-s0", 10, "incbcd", (15, 0, 8)),
    Case("incbcd-2digit-s2", 10, "incbcd", (42, 2, 8)),
    Case("decbcd-2digit-s0", 10, "decbcd", (15, 0, 8)),
    Case("decbcd-1digit-s4", 10, "decbcd", (3, 4, 4)),
    # ---- mul / div: carry register above and below the in/out register
    *_with_inverse("{}-carry-above", "mul", "div", (5, 0, 4, 4), reg(4, 4)),
    *_with_inverse("{}-carry-below", "mul", "div", (3, 5, 1, 4), reg(1, 4)),
    *_with_inverse("{}-s0-c9", "cmul", "cdiv", (5, 0, 4, 4, [9]), reg(4, 4)),
    *_with_inverse("{}-s1-c0-c9", "cmul", "cdiv", (5, 1, 5, 4, [0, 9]), reg(5, 4)),
    *_with_inverse("{}-carry-below-c0-c9", "cmul", "cdiv", (3, 5, 1, 4, [0, 9]), reg(1, 4)),
    *_with_inverse("{}-len3-c3-c9", "cmul", "cdiv", (7, 0, 4, 3, [3, 9]), reg(4, 3)),
    # ---- modular out-of-place ops; 13 < 2^4 leaves inputs >= N
    *_with_inverse("{}-n15-out-above", "mul_mod_n_out", "imul_mod_n_out", (7, 15, 0, 4, 4), reg(4, 4)),
    *_with_inverse("{}-n13-out-below", "mul_mod_n_out", "imul_mod_n_out", (5, 13, 5, 1, 4), reg(1, 4)),
    *_with_inverse("{}-n13-out-s6", "mul_mod_n_out", "imul_mod_n_out", (3, 13, 0, 6, 4), reg(6, 4)),
    Case("pow_mod_n_out-n15-out-above", 10, "pow_mod_n_out", (7, 15, 0, 4, 4), reg(4, 4)),
    Case("pow_mod_n_out-n13-out-below", 10, "pow_mod_n_out", (2, 13, 5, 1, 4), reg(1, 4)),
    Case("cmul_mod_n_out-n15-c8", 10, "cmul_mod_n_out", (7, 15, 0, 4, 4, [8]), reg(4, 4)),
    Case("cmul_mod_n_out-n15-c0-c9", 10, "cmul_mod_n_out", (7, 15, 1, 5, 4, [0, 9]), reg(5, 4)),
    Case("cmul_mod_n_out-n13-out-below-c0-c9", 10, "cmul_mod_n_out", (5, 13, 5, 1, 4, [0, 9]), reg(1, 4)),
    Case("cpow_mod_n_out-n15-c8", 10, "cpow_mod_n_out", (7, 15, 0, 4, 4, [8]), reg(4, 4)),
    Case("cpow_mod_n_out-n15-c0-c9", 10, "cpow_mod_n_out", (7, 15, 1, 5, 4, [0, 9]), reg(5, 4)),
    Case("cpow_mod_n_out-n13-out-below-c0-c9", 10, "cpow_mod_n_out", (2, 13, 5, 1, 4, [0, 9]), reg(1, 4)),
    # ---- indexed ops: value length 5 (one table byte) and 9 (two bytes)
    Case("indexed_lda-v5-above", 10, "indexed_lda", (0, 3, 4, 5, T8x1), reg(4, 5)),
    Case("indexed_lda-v5-below", 10, "indexed_lda", (6, 3, 0, 5, T8x1), reg(0, 5)),
    Case("indexed_lda-v9", 10, "indexed_lda", (0, 1, 1, 9, T2x2), reg(1, 9)),
    *_carry_pair("indexed_adc-v5-above", "indexed_adc", (0, 3, 4, 5, 9, T8x1), 9),
    *_carry_pair("indexed_adc-v5-below", "indexed_adc", (6, 3, 0, 5, 9, T8x1), 9),
    *_carry_pair("indexed_sbc-v5-above", "indexed_sbc", (0, 3, 4, 5, 9, T8x1), 9),
    *_carry_pair("indexed_sbc-v5-below-carry5", "indexed_sbc", (6, 3, 0, 5, 5, T8x1), 5),
    # ---- hash: random permutation tables of one and two bytes per entry
    Case("hash-s0", 10, "hash", (0, 4, HASH4)),
    Case("hash-s4", 10, "hash", (4, 4, HASH4)),
    Case("hash-len9", 10, "hash", (1, 9, HASH9)),
    # ---- rotations: shifts 1 and length-1
    Case("rol-1-s0", 10, "rol", (1, 0, 4)),
    Case("rol-3-s0", 10, "rol", (3, 0, 4)),
    Case("rol-1-s4", 10, "rol", (1, 4, 4)),
    Case("rol-3-s4", 10, "rol", (3, 4, 4)),
    Case("rol-9-full", 10, "rol", (9, 0, 10)),
    Case("ror-1-s0", 10, "ror", (1, 0, 4)),
    Case("ror-3-s4", 10, "ror", (3, 4, 4)),
    Case("ror-1-full", 10, "ror", (1, 0, 10)),
    # ---- phase flips
    Case("phase_flip_if_less-s0", 10, "phase_flip_if_less", (5, 0, 4)),
    Case("phase_flip_if_less-s4", 10, "phase_flip_if_less", (11, 4, 4)),
    Case("cphase_flip_if_less-flag9", 10, "cphase_flip_if_less", (5, 0, 4, 9)),
    Case("cphase_flip_if_less-flag0", 10, "cphase_flip_if_less", (11, 4, 4, 0)),
]

WIDE_CASES = [
    Case("w-inc", 13, "inc", (4099, 0, 13)),
    Case("w-cinc", 13, "cinc", (9, 4, 6, [0, 12])),
    *_carry_pair("w-incc", "incc", (37, 3, 6, 12), 12, n=13),
    *_with_inverse("w-{}", "cmul", "cdiv", (5, 2, 7, 4, [0, 12]), reg(7, 4), n=13),
    Case("w-cmul_mod_n_out", 13, "cmul_mod_n_out", (7, 13, 2, 7, 4, [0, 12]), reg(7, 4)),
    Case("w-cpow_mod_n_out", 13, "cpow_mod_n_out", (7, 15, 7, 2, 4, [0, 12]), reg(2, 4)),
    Case("w-indexed_lda-v9", 13, "indexed_lda", (0, 3, 4, 9, T8x2), reg(4, 9)),
    *_carry_pair("w-indexed_adc-v9", "indexed_adc", (0, 3, 3, 9, 12, T8x2), 12, n=13),
    *_carry_pair("w-indexed_sbc-v9", "indexed_sbc", (0, 3, 3, 9, 12, T8x2), 12, n=13),
    Case("w-hash-len9", 13, "hash", (3, 9, HASH9)),
    Case("w-rol", 13, "rol", (5, 3, 8)),
    Case("w-incbcd-3digit", 13, "incbcd", (123, 1, 12)),
]

# the four representative ops of the capped-grid (grid-stride loop) run
STRIDE_CASES = [
    Case("stride-inc", 10, "inc", (11, 4, 4)),
    Case("stride-cmul_mod_n_out", 10, "cmul_mod_n_out", (7, 15, 1, 5, 4, [0, 9]), reg(5, 4)),
    Case("stride-indexed_adc", 10, "indexed_adc", (0, 3, 4, 5, 9, T8x1), 1 << 9),
    Case("stride-rol", 10, "rol", (3, 4, 4)),
]


def case_ids(cases):
    return [c.id for c in cases]


def case_input(case, precision):
    """The op's input, already rounded to the engine's precision, as
    complex128 (the oracle's input) — the same for every engine."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    state = ao.random_state(case.n, rng, case.zero_mask)
    for name, args in case.pre:
        state = getattr(ao, name)(state, *args)
    return state.astype(DTYPE[precision]).astype(np.complex128)


def case_expected(case, state):
    return getattr(ao, case.op)(state, *case.args)


def apply_case(sim, case, state, precision):
    """Load `state`, run the op, read the state back."""
    sim.set_state_vector(state.astype(DTYPE[precision]))
    getattr(sim, case.op)(*case.args)
    return np.asarray(sim.get_state_vector())


def check_result(got, expected, precision, rescaled=False):
    """Bit-for-bit equality with the oracle, and unit norm to 8 eps.

    `rescaled` is for the ops that measure a carry qubit which the input
    holds in |1> (incc, decc, indexed_adc, indexed_sbc). The measurement
    collapses with a factor 1/sqrt(prob) (QEngine::ForceM in
    csrc/qengine.hpp, applied by ApplyM / k_applym), where prob is a
    reduction over the state that comes out as 1 up to a few eps, so every
    amplitude is rescaled by a factor a few eps from one before the
    permutation moves it. Those cases get |got - expected| <=
    4 eps |expected| elementwise, with expected zeros exactly zero. With the
    carry clear the probability of |1> sums exact zeros, the factor is
    exactly one, and the case stays bit for bit.
    """
    got = np.asarray(got)
    assert got.dtype == DTYPE[precision]
    norm2 = float(np.sum(np.abs(got.astype(np.complex128)) ** 2))
    print(f"norm^2 - 1 = {norm2 - 1.0:.3e}")
    assert abs(norm2 - 1.0) <= 8 * EPS[precision], f"norm^2 = {norm2!r}"
    want = expected.astype(DTYPE[precision])
    if rescaled:
        zero = want == 0
        assert not np.any(got[zero]), "amplitude in a slot the oracle leaves empty"
        err = np.abs(got.astype(np.complex128) - expected)
        ratio = (err[~zero] / np.abs(expected[~zero])).max() / EPS[precision]
        print(f"max |got - expected| / |expected| = {ratio:.2f} eps")
        assert np.all(err <= 4 * EPS[precision] * np.abs(expected)), f"{ratio:.2f} eps"
        return
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (
        f"{bad.size} amplitudes differ from the oracle; first at {bad[0]}: "
        f"got {got[bad[0]]!r}, expected {want[bad[0]]!r}; "
        f"max |diff| = {np.abs(got - want).max():.3e}"
    )


def run_case(sim, case, precision):
    state = case_input(case, precision)
    got = apply_case(sim, case, state, precision)
    check_result(got, case_expected(case, state), precision, case.rescaled)
