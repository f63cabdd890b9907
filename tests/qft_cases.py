"""Case table, input builder and checks shared by test_qft_oracle_cpu.py and
test_qft_oracle_gpu.py: the QFT family of an engine against qft_oracle.py.

Input: a fixed-seed complex Gaussian state (every amplitude distinct and
non-zero), normalised and rounded to the engine's dtype before either side
sees it, loaded with set_state_vector and read with get_state_vector. The
basis cases load phase |perm> through set_permutation(perm, phase) instead,
which the HIP engine keeps pending, so its lazy first-pass and
support-restricted kernels are held to the oracle too.

Reference: qft_oracle in np.clongdouble for every fp64 case and for every
case of width <= 17, np.complex128 for the wider fp32 ones (its error there,
about 21 * 2^-53, is 1e-8 of the fp32 tolerance). The fp64 cases need a long
double with eps < 2^-60 (qft_oracle.LONG_OK); where it is narrower they are
skipped with that reason.

Tolerance, asserted per case, P = the number of columns applied (`length`;
1 for a primitive, 2 for qft_column2_general), R the engine's real type:

    ||got - exp||_2  <= C * P * eps_R
    max |got - exp|  <= C * P * eps_R * max |exp|
    | ||got||^2 - 1 | <= 8 * P * eps_R

Every column is unitary, so the 2-norm of the rounding error of P columns is
at most the sum of the P per-column errors and does not grow with the state.

C for the CPU engine (both precisions) and the HIP engine in fp64 is derived,
to first order, u = eps / 2, in units of the state's norm:
- The H of a column: an add (u), the constant 1/sqrt(2) (off by at most u)
  and the product's rounding (u): 3 u = 1.5 eps.
- A complex multiply is off by sqrt(5) u = 1.12 eps of its magnitude.
- sincos is within one ulp per component, and one ulp of a value below 1 is
  at most u, so the unit complex number is off by at most sqrt(2) u =
  0.71 eps; its argument scale * frac carries the rounding of pi (in scale)
  and of the product, a relative 2 u = eps, so an absolute eps * angle.
- A lone column (k_qft_col, the ramp primitives): angle < pi, so the factor
  is off by pi + 0.71 = 3.85 eps, times one multiply: 1.5 + 3.85 + 1.12 =
  6.5 eps.
- A fused group of K columns (k_qft_colK, qftOrbitColumns, the CPU engine's
  QftColumn): one sincos f0 of an angle below pi / 2^(K-1), then
  fPow[m] = fPow[m-1]^2, so E_0 = pi / 2^(K-1) + 0.71 and
  E_m = 2 E_{m-1} + 1.12 eps. Slot column c (c = K-1 the highest) takes
  fPow[K-1-c] times up to c constant roots of unity, each another multiply
  (1.12) by a constant that is itself off by 0.71 eps: F_c = E_{K-1-c} +
  1.83 c. Per column that is 1.5 + F_c + 1.12; averaged over the group:
      K = 2: E = 2.28, 5.68         F = 5.68, 4.11         mean 4.90    7.5 eps
      K = 3: E = 1.50, 4.11, 9.34   F = 9.34, 5.94, 5.16   mean 6.81    9.4 eps
      K = 4: E = 1.10, 3.32, 7.77, 16.65
             F = 16.65, 9.60, 6.98, 6.59  mean 9.96   12.6 eps
      K = 5: E = 0.91, 2.93, 6.98, 15.08, 31.28
             F = 31.28, 16.91, 10.64, 8.42, 8.23  mean 15.10   17.7 eps
  A pass of several groups (low ladder, mid passes) costs each group the
  same, and a P-column transform is a sum of whole groups.
The costliest is K = 5 (QRACK_GPU_QFT_FUSE=5) at 17.7 eps per column, so

    C = 18.

The default schedules (K <= 4) stay below 12.6. Measured, the CPU engine
stays below 0.67 in the 2-norm and 1.5 element-wise (the single-column
primitives; the transforms below 0.5): the count above is a worst case that
lets every rounding error align.

The HIP engine in fp32 takes __sincosf in every kernel, whose error has no
documented bound; its C is measured on an MI355X (test_qft_oracle_gpu.py).

Condition on the tolerance, so that it cannot hide a dropped ladder term:
for every Gaussian-input case with `full_ladder` (all fp64 cases, fp32 cases
of length <= 13) the test computes floor = ||oracle - oracle(drop = the
smallest-angle term of the top column)||_2 and asserts C * P * eps <=
floor / 2.

Angles: the callers (QPager::QFT / IQFT, dist_pager._column_ramp) pass
scale = +-pi / 2^i, frac < 2^i and phase0 = scale * meta_weight, so every
angle lies in (-pi, pi); the primitive table covers both signs.

`plan` is the pass list the HIP engine must take, in the notation of
test_qft_pass_plan.py ("m12.2 l12"), written by hand; `routes_of` turns it
into profile_report() op counts.
"""

import functools
import zlib
from typing import NamedTuple, Optional

import numpy as np

import qft_oracle as qo

EPS = {"fp32": 2.0**-23, "fp64": 2.0**-52}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}
PRECISIONS = ("fp32", "fp64")
C_DERIVED = 18.0
ROUTE_OPS = ("qft_low_lds", "qft_mid_lds", "qft_column5", "qft_column4", "qft_column3",
             "qft_column2", "qft_column", "phase_ramp")
OPS = ("qft", "iqft")
LONG_SKIP = "long double of this machine is too narrow to referee fp64 (eps >= 2^-60)"


class Case(NamedTuple):
    id: str
    n: int
    start: int
    length: int
    plan: Optional[str] = None       # HIP engine's pass list, by hand
    basis: Optional[tuple] = None    # (perm, phase): input through set_permutation
    layers: Optional[tuple] = None   # outer layers over the engine
    qubits: Optional[tuple] = None   # qftr / iqftr over this list
    ops: tuple = OPS
    dft_ref: bool = False            # reference is qft_oracle.dft_bitrev


def _full(n, plan, **kw):
    return Case(f"n{n}", n, 0, n, plan, **kw)


def _sub(n, start, length, plan, **kw):
    return Case(f"n{n}-s{start}-l{length}", n, start, length, plan, **kw)


# ---- default switches ---------------------------------------------------------------

CASES = {
    "fp32": [
        _full(1, "c0.1"),
        _full(2, "c1.1 c0.1"),          # k_qft_col_v at tPow = 2
        _full(6, "c2.4 c0.2"),          # col2 scalar, tLo = 1
        _full(7, "c3.4 c0.3"),          # col3 scalar
        _full(10, "c6.4 c2.4 c0.2"),
        _full(11, "c7.4 c3.4 c0.3"),
        _full(12, "l12"),
        _full(13, "c12.1 l12"),         # one peeled column over the ladder
        _full(14, "m12.2 l12"),
        _full(15, "m12.3 l12"),
        _full(16, "m12.4 l12"),
        _full(17, "m8.9 l8"),           # the wide kernel
        _full(18, "m12.6 l12"),
        _full(19, "m13.6 c12.1 l12"),
        _full(20, "m12.8 l12"),
        _full(21, "m12.9 l12"),
        # spectators above the register
        _sub(12, 0, 8, "l8"),
        _sub(12, 0, 4, "l4"),
        _sub(14, 0, 12, "l12"),
        _sub(16, 0, 14, "m12.2 l12"),
        # start > 0: no LDS, register kernels with rampStart > 0
        _sub(10, 3, 6, "c2.4 c0.2"),    # col2_v and colK
        _sub(10, 3, 7, "c3.4 c0.3"),    # col3_v
        _sub(13, 1, 12, "c8.4 c4.4 c0.4"),
        _sub(16, 5, 11, "c7.4 c3.4 c0.3"),  # ends at the top bit
        _sub(14, 2, 1, "c0.1"),         # a bare H
        _sub(14, 13, 1, "c0.1"),
    ],
    "fp64": [
        _full(7, "c3.4 c0.3"),
        _full(10, "c6.4 c2.4 c0.2"),
        _full(11, "c9.2 l9"),
        _full(12, "c8.4 c6.2 l6"),
        _full(13, "c9.4 l9"),
        _full(14, "c10.4 c9.1 l9"),
        _sub(11, 0, 9, "l9"),
        _sub(11, 0, 6, "l6"),
        _sub(12, 0, 4, "c3.1 l3"),
        _sub(10, 3, 6, "c2.4 c0.2"),
        _sub(13, 1, 12, "c8.4 c4.4 c0.4"),
    ],
}

# the one wide case: Gaussian input, forward only, against the closed DFT form;
# its last pass is the tile-sums variant of the low ladder
CASES["fp32"].append(Case("n23-dft", 23, 0, 23, "m14.9 m8.6 l8", ops=("qft",), dft_ref=True))

# qftr / iqftr over a scattered list: the generic gate lowering
CASES["fp32"].append(Case("qftr-n10", 10, 0, 5, qubits=(7, 2, 9, 0, 4)))
CASES["fp64"].append(Case("qftr-n10", 10, 0, 5, qubits=(7, 2, 9, 0, 4)))


def _basis(n, length, plan):
    mask = (1 << n) - 1
    phase = complex(np.exp(0.7j))
    combos = (("zero", 0, 1.0 + 0j), ("ones", mask, phase),
              ("5a", 0x5A5A5A5A & mask, 1.0 + 0j), ("top", 1 << (n - 1), phase))
    tag = f"n{n}" if length == n else f"n{n}-s0-l{length}"
    return [Case(f"{tag}-basis-{name}", n, 0, length, plan, basis=(perm, ph))
            for name, perm, ph in combos]


# phase |perm>: full-width ones take the support-restricted schedule; the
# shorter registers stay pending into launchQftLowLdsBasis /
# launchQftMidLdsBasis with perm bits above the register
BASIS_CASES = {
    "fp32": (_basis(12, 12, "l12") + _basis(14, 14, "m12.2 l12") + _basis(17, 17, "m8.9 l8")
             + _basis(21, 21, "m12.9 l12") + _basis(14, 12, "l12")
             + _basis(16, 14, "m12.2 l12")),
    "fp64": _basis(11, 9, "l9") + _basis(12, 12, "c8.4 c6.2 l6") + _basis(13, 13, "c9.4 l9"),
}

# layers=["pager", <engine>] with pages_per_device=4: 14 qubits per page
PAGER_CASES = [
    Case("pager-n16", 16, 0, 16, layers=("pager",)),
    Case("pager-n16-s2-l13", 16, 2, 13, layers=("pager",)),   # straddles the page boundary
    Case("pager-n16-s14-l2", 16, 14, 2, layers=("pager",)),   # all meta
]
PAGES_PER_DEVICE = 4

TABLE = {p: CASES[p] + BASIS_CASES[p] for p in PRECISIONS}

# ---- switch children ------------------------------------------------------------------
# name -> (environment, qft_pass_plan keywords, {precision: [cases]})

_F1_10 = "c9.1 c8.1 c7.1 c6.1 c5.1 c4.1 c3.1 c2.1 c1.1 c0.1"
_F1_S3 = "c5.1 c4.1 c3.1 c2.1 c1.1 c0.1"


def _both(cases):
    return {"fp32": list(cases), "fp64": list(cases)}


SWITCHES = {
    # every column through k_qft_col_v / k_qft_col
    "fuse1": ({"QRACK_GPU_QFT_FUSE": "1"}, {"fuse": 1},
              _both([_full(10, _F1_10), _sub(10, 3, 6, _F1_S3)])),
    "fuse2": ({"QRACK_GPU_QFT_FUSE": "2"}, {"fuse": 2},
              _both([_full(10, "c8.2 c6.2 c4.2 c2.2 c0.2")])),
    "fuse3": ({"QRACK_GPU_QFT_FUSE": "3"}, {"fuse": 3},
              _both([_full(10, "c7.3 c4.3 c1.3 c0.1")])),
    # k_qft_colK<R, 5, *>
    "fuse5": ({"QRACK_GPU_QFT_FUSE": "5"}, {"fuse": 5},
              {"fp32": [_full(10, "c5.5 c0.5"), _full(11, "c6.5 c1.5 c0.1"),
                        _sub(12, 3, 8, "c3.5 c0.3")],
               "fp64": [_full(10, "c5.5 c0.5"), _full(11, "c9.2 l9"),
                        _sub(12, 3, 8, "c3.5 c0.3")]}),
    # k_qft_col_v_pipe
    "pipe": ({"QRACK_GPU_QFT_PIPE": "1", "QRACK_GPU_QFT_FUSE": "1"}, {"fuse": 1},
             {"fp32": [_full(10, _F1_10)], "fp64": []}),
    # register columns with 13-bit ramps
    "lds0": ({"QRACK_GPU_QFT_LDS": "0"}, {"lds_low": False},
             {"fp32": [_full(14, "c10.4 c6.4 c2.4 c0.2")],
              "fp64": [_full(13, "c9.4 c5.4 c1.4 c0.1")]}),
    "midlds0": ({"QRACK_GPU_QFT_MIDLDS": "0"}, {"lds_mid": False},
                {"fp32": [_full(14, "c10.4 c8.2 l8")], "fp64": []}),
    "midmax6": ({"QRACK_GPU_QFT_MIDMAX": "6"}, {"midmax": 6},
                {"fp32": [_full(17, "m11.6 c8.3 l8"), _full(19, "m13.6 c9.4 c8.1 l8")],
                 "fp64": []}),
}


def _by_id(cases, *ids):
    return [c for c in cases if c.id in ids]


# QRACK_GPU_BLOCKS=3: three blocks walk every tile loop, so the low ladder (4
# tiles at 14 qubits), the 2- to 6-column mid passes (64 down to 16 tiles) and
# the wide pass (16 tiles at 17 qubits) all take their later trips
SWITCHES["blocks3"] = (
    {"QRACK_GPU_BLOCKS": "3"}, {},
    {"fp32": (_by_id(CASES["fp32"], "n14", "n15", "n16", "n17", "n18")
              + [c for c in BASIS_CASES["fp32"]
                 if c.id.startswith(("n14-basis", "n17-basis", "n16-s0-l14-basis"))]),
     "fp64": _by_id(CASES["fp64"], "n13", "n14")})
# the default table again with the profiler on, for the declared routes
SWITCHES["profile"] = (
    {}, {},
    {p: [c for c in TABLE[p] if c.plan is not None and c.n <= 19] for p in PRECISIONS})


def all_cases(precision):
    out = list(TABLE[precision]) + list(PAGER_CASES)
    for _env, _kw, per in SWITCHES.values():
        out += per[precision]
    return out


# ---- inputs, references, checks ---------------------------------------------------------

def gaussian_state(tag, n, precision):
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (v / np.linalg.norm(v)).astype(DTYPE[precision])


def case_input(case, precision):
    """The state both sides start from, already in the engine's dtype."""
    if case.basis is not None:
        perm, phase = case.basis
        v = np.zeros(1 << case.n, dtype=DTYPE[precision])
        v[perm] = phase
        return v
    return gaussian_state(f"qft-n{case.n}", case.n, precision)


def uses_long(case, precision):
    return precision == "fp64" or case.n <= 17


def _expected_uncached(case, op, precision, drop=None):
    v = case_input(case, precision)
    inverse = op in ("iqft", "iqftr")
    if case.dft_ref:
        assert not inverse and drop is None
        return qo.dft_bitrev(v, case.n)
    w = qo.work(v, long=uses_long(case, precision))
    if case.qubits is not None:
        return qo.qftr(w, list(case.qubits), inverse)
    return qo.qft(w, case.start, case.length, inverse, drop)


@functools.lru_cache(maxsize=None)
def _expected_small(case, op, precision):
    out = _expected_uncached(case, op, precision)
    out.setflags(write=False)
    return out


def expected(case, op, precision):
    """The oracle's state, computed once per (case, op, precision) up to 19
    qubits and shared read-only; the few wider ones are used once each."""
    if case.n <= 19:
        return _expected_small(case, op, precision)
    return _expected_uncached(case, op, precision)


def load(q, case, precision):
    if case.basis is not None:
        q.set_permutation(case.basis[0], case.basis[1])
    else:
        q.set_state_vector(case_input(case, precision))


def apply(q, case, op):
    if case.qubits is not None:
        getattr(q, op + "r")(list(case.qubits))
    else:
        getattr(q, op)(case.start, case.length)


def run(q, case, op, precision):
    """Load the case's input, apply op, return the engine's state."""
    load(q, case, precision)
    apply(q, case, op)
    return np.asarray(q.get_state_vector())


def errors(got, exp):
    """(2-norm of the difference, max difference / max |exp|, | ||got||^2 - 1 |)
    taken in the reference's dtype."""
    g = np.asarray(got).astype(exp.dtype)
    d = np.abs(g - exp)
    two = float(np.sqrt(np.sum(d * d)))
    mx = float(d.max() / np.abs(exp).max())
    nrm = float(abs(np.sum(np.abs(g) ** 2) - 1))
    return two, mx, nrm


def check(got, exp, precision, cols, c=C_DERIVED, label=""):
    """Print the figures in units of cols * eps, then assert them."""
    assert got.shape == exp.shape and got.dtype == DTYPE[precision]
    unit = cols * EPS[precision]
    two, mx, nrm = errors(got, exp)
    print(f"{label} {precision}: 2-norm {two / unit:.3f}, max {mx / unit:.3f}, "
          f"norm {nrm / unit:.3f} (P eps), bound {c:g} / {c:g} / 8")
    assert two <= c * unit, (label, "2-norm", two / unit, c)
    assert mx <= c * unit, (label, "max", mx / unit, c)
    assert nrm <= 8 * unit, (label, "norm", nrm / unit)
    return two / unit, mx / unit


def full_ladder(case, precision):
    """Gaussian-input cases only: on a basis state a phase whose control is
    clear changes nothing, so there the floor can be zero."""
    return case.qubits is None and not case.dft_ref and case.basis is None and (
        precision == "fp64" or case.length <= 13) and case.length >= 2


def drop_distance(case, op, precision, ctrl=0):
    """|| oracle - oracle without the top column's phase controlled by bit
    start + ctrl ||_2: what losing that one ladder term moves the state by."""
    full = expected(case, op, precision)
    less = _expected_uncached(case, op, precision, drop=(case.length - 1, ctrl))
    d = np.abs(full - less)
    return float(np.sqrt(np.sum(d * d)))


def check_floor(case, op, precision, c):
    """The tolerance must sit at or below half the smallest dropped term."""
    floor = drop_distance(case, op, precision)
    tol = c * case.length * EPS[precision]
    print(f"{case.id} {op} {precision}: tolerance {tol:.3e}, dropped-term floor {floor:.3e}")
    assert tol <= floor / 2, (case.id, op, tol, floor)


def detectable_ctrl(case, op, precision, c):
    """Unflagged cases: the lowest control of the top column whose removal
    the tolerance still detects (floor / 2 >= tolerance), or None."""
    tol = c * case.length * EPS[precision]
    for ctrl in range(case.length - 1):
        if drop_distance(case, op, precision, ctrl) / 2 >= tol:
            return ctrl
    return None


# ---- plans and routes ------------------------------------------------------------------

def parse_plan(text):
    kinds = {"l": "low", "m": "mid", "c": "col"}
    plan = []
    for tok in text.split():
        if tok[0] == "l":
            plan.append(("low", 0, int(tok[1:])))
        else:
            lo, nc = tok[1:].split(".")
            plan.append((kinds[tok[0]], int(lo), int(nc)))
    return plan


def routes_of(plan_text):
    """profile_report() op counts of one walk of the plan; column 0 alone is
    an H through the gate path and counts as none of them."""
    out = {}
    for kind, lo, nc in parse_plan(plan_text):
        if kind == "low":
            op = "qft_low_lds"
        elif kind == "mid":
            op = "qft_mid_lds"
        elif nc > 1:
            op = f"qft_column{nc}"
        elif lo > 0:
            op = "qft_column"
        else:
            continue
        out[op] = out.get(op, 0) + 1
    return out


# ---- ramp primitives --------------------------------------------------------------------

class Prim(NamedTuple):
    id: str
    n: int
    op: str
    args: tuple
    cols: int = 1
    hip_only: bool = False


def _prims():
    out = []
    pi = float(np.pi)
    # phase_ramp(scale, ramp_start, ramp_bits, cond_pow): 5 ramp bits;
    # cond_pow 1 is the scalar fp32 kernel
    for rs in (0, 3):
        for cond in (0, 1, 2, 1 << 9):
            for sign in (1, -1):
                out.append(Prim(f"ramp-rs{rs}-c{cond}-{'p' if sign > 0 else 'm'}", 10,
                                "phase_ramp", (sign * pi / 32, rs, 5, cond)))
    # phase_ramp_general(scale, ramp_start, in_place_mask, pows, weights,
    # cond_pow) with 0, 2, 8 and 9 relocated bits (9: the host fallback of
    # the HIP engine); frac < 2^i and scale = +-pi / 2^i
    reloc = {
        0: (pi / 32, 2, 0b11111, (), ()),
        2: (pi / 128, 0, 0b1011, (1 << 6, 1 << 8), (16, 64)),
        8: (pi / 512, 0, 0b1, tuple(1 << b for b in (1, 2, 3, 5, 6, 7, 8, 9)),
            (64, 2, 128, 8, 256, 4, 32, 16)),
        9: (pi / 512, 0, 0, tuple(1 << b for b in (0, 1, 2, 3, 5, 6, 7, 8, 9)),
            (64, 2, 128, 8, 256, 4, 32, 16, 1)),
    }
    for k, (scale, rs, mask, pows, ws) in reloc.items():
        for cond in (0, 1 << 4):
            for sign in (1, -1):
                out.append(Prim(f"rampgen-k{k}-c{cond}-{'p' if sign > 0 else 'm'}", 10,
                                "phase_ramp_general",
                                (sign * scale, rs, mask, list(pows), list(ws), cond)))
    # qft_column_general(target, scale, ramp_start, in_place_mask, pows,
    # weights, phase0, pre): target 0 is the scalar fp32 kernel; the ramp
    # bits (1, 2, 3 in place, 6 and 8 relocated) avoid every target; the
    # inverse order (pre) takes the negative angles, as the callers do
    for t in (0, 4, 9):
        for pre in (False, True):
            for p0 in (0.0, 0.3):
                sign = -1 if pre else 1
                out.append(Prim(f"colgen-t{t}-{'pre' if pre else 'post'}-p{p0:g}", 10,
                                "qft_column_general",
                                (t, sign * pi / 128, 0, 0b1110, [1 << 6, 1 << 8], [16, 64],
                                 sign * p0, pre)))
    # qft_column2_general(target_hi, target_lo, scale_hi, ...): logical
    # columns 9 and 8 on slots 4 and 7, the shape test_dist_pager_gpu.py uses
    for pre in (False, True):
        sign = -1 if pre else 1
        out.append(Prim(f"col2gen-{'pre' if pre else 'post'}", 12, "qft_column2_general",
                        (4, 7, sign * pi / 512, 0, 0b1011, [1 << 6, 1 << 10], [16, 64],
                         sign * 0.21, sign * 0.42, pre), cols=2, hip_only=True))
    return out


PRIMS = _prims()
PRIM_BY_ID = {p.id: p for p in PRIMS}


def prim_input(prim, precision):
    return gaussian_state(f"prim-n{prim.n}", prim.n, precision)


def round_scale(x, precision):
    """The bindings take phase_ramp's scale in the engine's real type."""
    return float(np.float32(x)) if precision == "fp32" else float(x)


def prim_args(prim, precision):
    """The arguments as the engine receives them: phase_ramp and
    phase_ramp_general take their scale in the engine's real type, so both
    sides get the rounded value; the column primitives take doubles."""
    if prim.op in ("phase_ramp", "phase_ramp_general"):
        return (round_scale(prim.args[0], precision),) + tuple(prim.args[1:])
    return tuple(prim.args)


@functools.lru_cache(maxsize=None)
def prim_expected(prim_id, precision):
    prim = PRIM_BY_ID[prim_id]
    w = qo.work(prim_input(prim, precision))
    a = prim_args(prim, precision)
    if prim.op == "qft_column2_general":
        t_hi, t_lo, scale, rs, mask, pows, ws, p0h, p0l, pre = a
        # the two general columns it fuses: the high column's ramp also
        # takes the low target's bit, at the weight that makes its angle pi / 2
        hi = (t_hi, scale, rs, mask, pows + [1 << t_lo], ws + [1 << 8], p0h)
        lo = (t_lo, 2 * scale, rs, mask, pows, ws, p0l)
        for col in ((lo, hi) if pre else (hi, lo)):
            qo.qft_column_general(w, *col, pre)
    else:
        getattr(qo, prim.op)(w, *a)
    w.setflags(write=False)
    return w


def run_prim(q, prim, precision):
    q.set_state_vector(prim_input(prim, precision))
    getattr(q, prim.op)(*prim_args(prim, precision))
    return np.asarray(q.get_state_vector())
