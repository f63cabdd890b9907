"""Case table, input builder and checks shared by test_gate_oracle_cpu.py and
test_gate_oracle_gpu.py: the gate path of an engine against gate_oracle.py.

Input: a fixed-seed complex Gaussian state (every amplitude distinct and
non-zero), normalised and rounded to the engine's dtype, loaded with
set_state_vector and read back with get_state_vector. Matrices, and the
angles of fsim / phase_parity, are rounded to the engine's dtype before
either side sees them, so the oracle and the engine apply the same numbers.

Tolerance (derived, not measured), elementwise:

    |got_i - exp_i| <= c * G * eps_R * a_i

G is the number of matrices the oracle applied and a_i the oracle's
companion vector (|v| pushed through |M|: it bounds every partial sum that
forms amplitude i). c = 3, plus 1 where the engine itself forms matrix
entries from an angle in precision R (fsim, fsim_batch, phase_parity).
To first order, with u = eps/2: a complex multiply is off by at most
sqrt(5) u of its magnitude, and a d-term sum adds (d - 1) u, so one 2x2 row
costs (sqrt(5) + 1) u = 1.62 eps and one 4x4 row (sqrt(5) + 3) u = 2.62 eps
of a_i; the MFMA form of a 2x2 (a real 4x4 row per component, combined in
quadrature over re and im) costs 4 sqrt(2) u = 2.83 eps. All are below
3 eps, and G gates add up to G times that of the final a_i because a_i is
carried through the same |M|. An entry formed as polar(1, angle) or
cos / sin in precision R is within one eps of the oracle's, which is the
extra 1.

Unitary cases (all of them) also assert | ||got||^2 - 1 | <= 8 G eps_R.

Value-exact ops (x, cnot, ccnot, anti_cnot, swap, cswap, x_mask, y_mask,
z_mask, z, cz, cnot_batch, and any diagonal whose entries are all 1) only
move, negate or swap components, so they are asserted with np.array_equal.

The fp32 cphase_pairs kernel of the HIP engine takes a native sincos of
the summed angle, whose error has no documented bound; cases flagged
`native_sincos` accept a measured relative tolerance there instead (see
test_gate_oracle_gpu.py). Everywhere else they use the derived bound.

`routes` (batch cases) is the host dispatch the HIP engine must take, as
profile_report() op counts per precision.
"""

import zlib
from typing import NamedTuple, Optional

import numpy as np

import gate_oracle as go

EPS = {"fp32": 2.0**-23, "fp64": 2.0**-52}
DTYPE = {"fp32": np.complex64, "fp64": np.complex128}
REAL = {"fp32": np.float32, "fp64": np.float64}
PRECISIONS = ("fp32", "fp64")
# qaLdsTileBits<R>(): batches fuse through the LDS kernels when the state is
# wider than this and the targets sit below it
TILE_BITS = {"fp32": 12, "fp64": 11}
ROUTE_OPS = (
    "mtrx_1q_batch_lds", "mtrx_1q_batch", "mtrx_2q_batch_lds", "mtrx_2q_pair2", "mtrx_2q",
    "fsim_batch_lds", "cphase_pairs", "cnot_batch", "apply2x2",
)
ANGLE_OPS = ("fsim", "fsim_batch", "phase_parity")


class Case(NamedTuple):
    id: str
    n: int
    op: str
    args: tuple
    exact: bool = False
    routes: Optional[dict] = None
    native_sincos: bool = False


def _rng(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def _unitary(rng, dim):
    z = rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))
    q, r = np.linalg.qr(z)
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _phase(rng):
    return np.exp(1j * rng.uniform(0.3, 2 * np.pi - 0.3))


def _round_c(x, precision):
    return np.asarray(x, dtype=np.complex128).astype(DTYPE[precision]).astype(np.complex128)


def _round_r(x, precision):
    return [float(v) for v in np.asarray(x, dtype=np.float64).astype(REAL[precision])]


def _clist(x, precision):
    return [complex(v) for v in _round_c(x, precision).ravel()]


# ---- Apply2x2 family ---------------------------------------------------------

KINDS = ("unitary", "diag", "diag1b", "diaga1", "identity", "antidiag", "x")


def _gate_case(name, n, kind, t, controls, anti, precision):
    """One of the seven matrices through the method family its shape has."""
    cid = f"{name}-{kind}-t{t}-{'a' if anti else 'c'}{''.join(map(str, controls)) or 'none'}"
    rng = _rng(cid)
    ctl = bool(controls)
    pre = ("mac" if anti else "mc") if ctl else ""
    head = (list(controls),) if ctl else ()
    if kind in ("unitary", "identity"):
        m = _unitary(rng, 2) if kind == "unitary" else np.eye(2)
        return Case(cid, n, pre + "mtrx", head + (_clist(m, precision), t), exact=kind == "identity")
    if kind in ("diag", "diag1b", "diaga1"):
        tl = 1.0 if kind == "diag1b" else _phase(rng)
        br = 1.0 if kind == "diaga1" else _phase(rng)
        tl, br = _clist([tl, br], precision)
        return Case(cid, n, pre + "phase", head + (tl, br, t))
    tr, bl = (1.0, 1.0) if kind == "x" else (_phase(rng), _phase(rng))
    tr, bl = _clist([tr, bl], precision)
    return Case(cid, n, pre + "invert", head + (tr, bl, t), exact=kind == "x")


def _apply2x2_cases(precision):
    out = []
    # 10 qubits: targets 0, 1, 5, 9; control sets on bit 0, bit 1, the top
    # bit, both ends and the middle, as controls and as anti-controls
    for t in (0, 1, 5, 9):
        sets = [()]
        for cs in ([0], [1], [9], [0, 9], [2, 7]):
            if t in cs:
                if cs == [9]:
                    cs = [8]
                elif cs == [0, 9] and t == 9:
                    cs = [0, 8]
                else:
                    continue
            sets.append(tuple(cs))
        for cs in sets:
            for anti in ((False, True) if cs else (False,)):
                for kind in KINDS:
                    out.append(_gate_case("g10", 10, kind, t, cs, anti, precision))
    # degenerate grids: maxI == 1, and odd maxI
    for kind in KINDS:
        out.append(_gate_case("g1", 1, kind, 0, (), False, precision))
        for c, t in ((0, 1), (1, 0)):
            for anti in (False, True):
                out.append(_gate_case("g2", 2, kind, t, (c,), anti, precision))
        for t in (0, 1, 2):
            cs = tuple(q for q in range(3) if q != t)
            for anti in (False, True):
                out.append(_gate_case("g3", 3, kind, t, cs, anti, precision))
        # 3 qubits, no control and one control: maxI == 4 and maxI == 2
        out.append(_gate_case("g3", 3, kind, 2, (), False, precision))
        out.append(_gate_case("g3", 3, kind, 1, (0,), False, precision))
    # the named value-exact gates
    out += [
        Case("x-t0", 10, "x", (0,), exact=True),
        Case("x-t9", 10, "x", (9,), exact=True),
        Case("z-t0", 10, "z", (0,), exact=True),
        Case("z-t5", 10, "z", (5,), exact=True),
        Case("cnot-c0-t9", 10, "cnot", (0, 9), exact=True),
        Case("cnot-c9-t0", 10, "cnot", (9, 0), exact=True),
        Case("cnot-c4-t3", 10, "cnot", (4, 3), exact=True),
        Case("anti_cnot-c0-t5", 10, "anti_cnot", (0, 5), exact=True),
        Case("anti_cnot-c7-t0", 10, "anti_cnot", (7, 0), exact=True),
        Case("ccnot-c0-c9-t5", 10, "ccnot", (0, 9, 5), exact=True),
        Case("ccnot-c2-c7-t0", 10, "ccnot", (2, 7, 0), exact=True),
        Case("ccnot-n3-t1", 3, "ccnot", (0, 2, 1), exact=True),
        Case("cz-c0-t9", 10, "cz", (0, 9), exact=True),
        Case("cz-c6-t1", 10, "cz", (6, 1), exact=True),
        Case("cz-n2", 2, "cz", (1, 0), exact=True),
    ]
    return out


# ---- composites with offset1 != 0 ---------------------------------------------

def _composite_cases(precision):
    out = []
    pairs = [(10, 0, 1), (10, 0, 9), (10, 3, 7), (10, 7, 3), (10, 8, 9), (2, 0, 1)]
    for n, q1, q2 in pairs:
        tag = f"n{n}-{q1}-{q2}"
        out.append(Case(f"swap-{tag}", n, "swap", (q1, q2), exact=True))
        out.append(Case(f"iswap-{tag}", n, "iswap", (q1, q2)))
        out.append(Case(f"sqrt_swap-{tag}", n, "sqrt_swap", (q1, q2)))
        th, ph = _round_r(_rng(f"fsim-{tag}").uniform(-3, 3, 2), precision)
        out.append(Case(f"fsim-{tag}", n, "fsim", (th, ph, q1, q2)))
        if n == 2:
            continue  # no room for a control
        for cs in ([5], [0, 9] if 0 not in (q1, q2) and 9 not in (q1, q2) else [2, 6]):
            ctag = "".join(map(str, cs))
            out.append(Case(f"cswap-{tag}-c{ctag}", n, "cswap", (list(cs), q1, q2), exact=True))
            out.append(Case(f"csqrt_swap-{tag}-c{ctag}", n, "csqrt_swap", (list(cs), q1, q2)))
    return out


# ---- mtrx_1q_batch -------------------------------------------------------------

def _reg_route(k):
    """Register path of k distinct targets: chunks of four, a lone leftover
    through the plain pair kernel."""
    r = {"mtrx_1q_batch": k // 4 + (1 if k % 4 >= 2 else 0)}
    if k % 4 == 1:
        r["apply2x2"] = 1
    return r


def _b1(cid, n, targets, routes, precision, ms=None):
    rng = _rng(cid)
    if ms is None:
        ms = [_unitary(rng, 2) for _ in targets]
    return Case(cid, n, "mtrx_1q_batch", (list(targets), _clist(ms, precision)), routes=routes)


def _batch1q_cases(precision):
    tb = TILE_BITS[precision]
    out = [
        _b1("b1-n2-01", 2, [0, 1], _reg_route(2), precision),
        _b1("b1-n3-12", 3, [1, 2], _reg_route(2), precision),
        _b1("b1-n3-02", 3, [0, 2], _reg_route(2), precision),
        _b1("b1-n5-1234", 5, [1, 2, 3, 4], _reg_route(4), precision),
        # float4 path in fp32
        _b1("b1-n10-37", 10, [3, 7], _reg_route(2), precision),
        _b1("b1-n10-259", 10, [2, 5, 9], _reg_route(3), precision),
        _b1("b1-n10-1469", 10, [1, 4, 6, 9], _reg_route(4), precision),
        # bit 0: scalar path
        _b1("b1-n10-04", 10, [0, 4], _reg_route(2), precision),
        _b1("b1-n10-038", 10, [0, 3, 8], _reg_route(3), precision),
        _b1("b1-n10-0129", 10, [0, 1, 2, 9], _reg_route(4), precision),
        _b1("b1-n10-range7", 10, list(range(7)), _reg_route(7), precision),
        _b1("b1-n10-13579", 10, [1, 3, 5, 7, 9], _reg_route(5), precision),
        _b1("b1-n10-926-unsorted", 10, [9, 2, 6], _reg_route(3), precision),
        # duplicate target, non-commuting matrices: sequential fallback
        _b1("b1-n10-33-duplicate", 10, [3, 3], {"apply2x2": 2}, precision),
    ]
    # the LDS kernel: 13 qubits for both precisions, and 12 qubits, where
    # fp64 (11 tile bits) is past the boundary and fp32 (12) is on it
    low_sets = {
        "01": [0, 1],
        "0-top": [0, tb - 1],
        "k3": [0, 4, tb - 1],
        "k5": [0, 1, 3, 6, tb - 1],
        "k7": [0, 1, 2, 4, 6, 8, tb - 1],
        "k9": [0, 1, 2, 3, 4, 5, 7, 9, tb - 1],
        "all": list(range(tb)),
    }
    for n in (13, 12):
        lds = n > tb
        for name, ts in low_sets.items():
            for shuffled in (False, True):
                cid = f"b1-n{n}-lds-{name}" + ("-shuffled" if shuffled else "")
                if shuffled:
                    ts = [int(t) for t in _rng(cid + "/order").permutation(ts)]
                routes = {"mtrx_1q_batch_lds": 1} if lds else _reg_route(len(ts))
                out.append(_b1(cid, n, ts, routes, precision))
    out += [
        _b1("b1-n13-mixed-0-5-top-TB", 13, [0, 5, tb - 1, tb],
            {"mtrx_1q_batch_lds": 1, "apply2x2": 1}, precision),
        _b1("b1-n13-mixed-3-12", 13, [3, 12], {"apply2x2": 2}, precision),
        _b1("b1-n14-mixed-012-12-13", 14, [0, 1, 2, 12, 13],
            {"mtrx_1q_batch_lds": 1, "mtrx_1q_batch": 1}, precision),
    ]
    return out


# ---- mtrx_2q, mtrx_2q_batch, fsim_batch ----------------------------------------

def _low_pairs(precision, count):
    """`count` disjoint pairs below the tile, bit 0 and the tile's top bit
    included, both orientations, qubit 5 left free for the straddling pair."""
    tb = TILE_BITS[precision]
    pairs = [(0, tb - 1), (3, 1), (2, 4), (7, 6), (8, 9)]
    pairs.append((10, 5) if tb == 12 else None)
    pairs = [p for p in pairs if p]
    return pairs[:count]


def _pair_sets(precision):
    """(name, n, pairs, routes of mtrx_2q_batch, routes of fsim_batch)."""
    nmax = 6 if precision == "fp32" else 5
    lds2, ldsf = {"mtrx_2q_batch_lds": 1}, {"fsim_batch_lds": 1}
    one, two = {"mtrx_2q": 1}, {"mtrx_2q_pair2": 1}
    # the maximum set uses qubit 5 in fp32, so the straddling sets take one less
    few = _low_pairs(precision, 2)
    many = _low_pairs(precision, 5)
    return [
        ("n10-1pair", 10, [(2, 6)], one, one),
        ("n10-2pairs", 10, [(0, 9), (4, 5)], two, two),
        ("n10-3pairs", 10, [(1, 8), (2, 3), (9, 0)], {**two, **one}, {**two, **one}),
        ("n10-swapped", 10, [(9, 0), (5, 4)], two, two),
        ("n10-mixed-orientation", 10, [(7, 1), (2, 8)], two, two),
        ("n4-01-23", 4, [(0, 1), (2, 3)], two, two),
        ("n4-30-12", 4, [(3, 0), (1, 2)], two, two),
        ("n10-chained", 10, [(0, 1), (1, 2)], {"mtrx_2q": 2}, {"mtrx_2q": 2}),
        ("n13-lds-1", 13, _low_pairs(precision, 1), lds2, ldsf),
        ("n13-lds-2", 13, few, lds2, ldsf),
        ("n13-lds-max", 13, _low_pairs(precision, nmax), lds2, ldsf),
        ("n13-lds-straddle", 13, many[:4] + [(5, 12)], {**lds2, **one}, {**ldsf, **one}),
        # (5,12) and (13,12) share qubit 12: the whole batch is sequential
        ("n14-lds-straddle-shared", 14, few + [(5, 12), (13, 12)], {"mtrx_2q": 4}, {"mtrx_2q": 4}),
        # two disjoint straddling pairs: one pair2 pass after the LDS pass
        ("n14-lds-straddle-2", 14, many[:4] + [(5, 12), (13, 9)], {**lds2, **two}, {**ldsf, **two}),
    ]


def _batch2q_cases(precision):
    out = []
    for n, q1, q2 in [(2, 0, 1), (2, 1, 0), (10, 0, 1), (10, 1, 0), (10, 0, 9), (10, 9, 0),
                      (10, 4, 5), (10, 8, 9), (10, 9, 8)]:
        cid = f"m2q-n{n}-{q1}-{q2}"
        out.append(Case(cid, n, "mtrx_2q", (_clist(_unitary(_rng(cid), 4), precision), q1, q2),
                        routes={"mtrx_2q": 1}))
    for name, n, pairs, r2, rf in _pair_sets(precision):
        q1s, q2s = [p[0] for p in pairs], [p[1] for p in pairs]
        cid = f"m2qb-{name}"
        rng = _rng(cid)
        ms = [_unitary(rng, 4) for _ in pairs]
        out.append(Case(cid, n, "mtrx_2q_batch", (_clist(ms, precision), q1s, q2s), routes=r2))
        cid = f"fsimb-{name}"
        rng = _rng(cid)
        th = _round_r(rng.uniform(-3, 3, len(pairs)), precision)
        ph = _round_r(rng.uniform(-3, 3, len(pairs)), precision)
        out.append(Case(cid, n, "fsim_batch", (th, ph, q1s, q2s), routes=rf))
    return out


# ---- cphase_pairs, cz_batch, cnot_batch ----------------------------------------

def _cphase_cases(precision):
    def cp(cid, n, pairs, angles):
        k = len(pairs)
        kernel = 1 <= k <= 16
        return Case(cid, n, "cphase_pairs",
                    ([p[0] for p in pairs], [p[1] for p in pairs], [float(a) for a in angles]),
                    routes={"cphase_pairs": 1} if kernel else {"apply2x2": k}, native_sincos=kernel)

    def pairs_of(cid, k):
        rng = _rng(cid)
        ps = []
        while len(ps) < k:
            c, t = (int(q) for q in rng.choice(10, 2, replace=False))
            ps.append((c, t))
        # angles exactly representable in fp32, so both engines see the same
        return ps, [float(np.float32(a)) for a in rng.uniform(-3, 3, k)]

    out = [cp("cp-n2", 2, [(0, 1)], [0.75])]
    for k in (1, 4, 16, 17):
        cid = f"cp-n10-k{k}"
        out.append(cp(cid, 10, *pairs_of(cid, k)))
    out += [
        cp("cp-n10-shared", 10, [(0, 1), (0, 2), (1, 2)], [0.5, -1.25, 2.0]),
        cp("cp-n10-twice", 10, [(3, 8), (3, 8)], [0.625, 1.5]),
        cp("cp-n10-cancel", 10, [(4, 0), (4, 0)], [0.8125, -0.8125]),
        cp("cp-n10-angles", 10, [(0, 9), (1, 5), (7, 2), (8, 3)], [0.0, np.pi, -1.3, 2.5]),
    ]
    # 0, pi, -1.3 and 50.0 one pair at a time. The fused op adds the angles of
    # the pairs an index satisfies before it takes one sincos, and an addition
    # near 50 is off by up to ulp(50)/2 = 16 eps_R of phase in any precision R,
    # which no per-gate bound in eps_R * a_i can cover; so the large angle is
    # not summed with others here, where the bound is about the kernel's own
    # arithmetic.
    for name, ang in (("0", 0.0), ("pi", np.pi), ("m1.3", -1.3), ("50", 50.0)):
        out.append(cp(f"cp-n10-angle-{name}", 10, [(2, 8)], [ang]))

    def cz(cid, n, pairs):
        return Case(cid, n, "cz_batch", ([p[0] for p in pairs], [p[1] for p in pairs]),
                    routes={"cphase_pairs": 1}, native_sincos=True)

    out += [
        cz("czb-n2", 2, [(0, 1)]),
        cz("czb-n10-k1", 10, [(9, 0)]),
        cz("czb-n10-k4", 10, [(0, 5), (1, 6), (7, 2), (9, 8)]),
        cz("czb-n10-shared", 10, [(0, 1), (0, 2), (1, 2)]),
    ]
    return out


def _cnot_cases(precision):
    def cn(cid, n, pairs, routes):
        return Case(cid, n, "cnot_batch", ([p[0] for p in pairs], [p[1] for p in pairs]),
                    exact=True, routes=routes)

    one = {"cnot_batch": 1}
    return [
        cn("cnb-n2-01", 2, [(0, 1)], one),
        cn("cnb-n2-10", 2, [(1, 0)], one),
        cn("cnb-n10-k1", 10, [(3, 6)], one),
        cn("cnb-n10-k3-no-bit0", 10, [(1, 7), (8, 2), (5, 4)], one),
        cn("cnb-n10-bit0-control", 10, [(0, 6), (9, 3)], one),
        cn("cnb-n10-bit0-target", 10, [(6, 0), (3, 9)], one),
        cn("cnb-n10-k5-all", 10, [(0, 9), (8, 1), (2, 3), (5, 4), (6, 7)], one),
        cn("cnb-n10-chained", 10, [(0, 1), (1, 2)], {"apply2x2": 2}),
        cn("cnb-n10-empty", 10, [], {}),
    ]


# ---- mask gates and the multiplexer ----------------------------------------------

def _mask_cases(precision):
    out = []
    for n in (1, 10):
        masks = {"zero": 0, "bit0": 1, "top": 1 << (n - 1), "all": (1 << n) - 1}
        if n == 10:
            masks["random"] = 0b1001101010
        for name, mask in masks.items():
            for op in ("x_mask", "y_mask", "z_mask"):
                out.append(Case(f"{op}-n{n}-{name}", n, op, (mask,), exact=True))
            r = _round_r([_rng(f"pp-{n}-{name}").uniform(-3, 3)], precision)[0]
            out.append(Case(f"phase_parity-n{n}-{name}", n, "phase_parity", (r, mask)))
    return out


def _mux_cases(precision):
    def mux(cid, n, controls, t):
        rng = _rng(cid)
        ms = [_unitary(rng, 2) for _ in range(1 << len(controls))]
        arr = _round_c(ms, precision).reshape(-1)
        return Case(cid, n, "uniformly_controlled_single_bit", (list(controls), t, arr))

    return [
        mux("mux-n2-c0-t1", 2, [0], 1),
        mux("mux-n2-c1-t0", 2, [1], 0),
        mux("mux-n10-c13-t0", 10, [1, 3], 0),
        mux("mux-n10-c09-t5", 10, [0, 9], 5),
        mux("mux-n10-c924-t0", 10, [9, 2, 4], 0),
        mux("mux-n10-c7031-t8", 10, [7, 0, 3, 1], 8),
    ]


def build_cases(precision):
    return (_apply2x2_cases(precision) + _composite_cases(precision) + _batch1q_cases(precision)
            + _batch2q_cases(precision) + _cphase_cases(precision) + _cnot_cases(precision)
            + _mask_cases(precision) + _mux_cases(precision))


CASES = {p: build_cases(p) for p in PRECISIONS}
IDS = [c.id for c in CASES["fp32"]]
assert IDS == [c.id for c in CASES["fp64"]] and len(set(IDS)) == len(IDS)
BY_ID = {p: {c.id: c for c in CASES[p]} for p in PRECISIONS}


# ---- capped-grid cases: 14 qubits, so that with two blocks of 256 threads every
# gate kernel's stride loop, and the tile loop of both LDS kernels, runs again ---

def build_stride_cases(precision):
    rng = _rng("stride")
    u2 = lambda: _clist(_unitary(rng, 2), precision)  # noqa: E731
    b = _clist([_phase(rng)], precision)[0]
    tr, bl = _clist([_phase(rng), _phase(rng)], precision)
    n = 14
    low = _low_pairs(precision, 3)
    th = _round_r(rng.uniform(-3, 3, 3), precision)
    ph = _round_r(rng.uniform(-3, 3, 3), precision)
    return [
        # k_apply2x2 (fp64 always; fp32 with a control on bit 0)
        Case("s-mtrx-t5", n, "mtrx", (u2(), 5)),                   # _1v, p > 1
        Case("s-mtrx-t0", n, "mtrx", (u2(), 0)),                   # _1v, p == 1
        Case("s-invert-t9", n, "invert", (tr, bl, 9)),
        Case("s-mcmtrx-c0-t5", n, "mcmtrx", ([0], u2(), 5)),       # k_apply2x2
        Case("s-mcmtrx-c7-t3", n, "mcmtrx", ([7], u2(), 3)),       # _v
        Case("s-mcphase-c0-t5", n, "mcphase", ([0], 1.0 + 0j, b, 5)),   # k_scale_side
        Case("s-mcphase-c7-t3", n, "mcphase", ([7], 1.0 + 0j, b, 3)),   # k_scale_side_v
        Case("s-swap-3-11", n, "swap", (3, 11), exact=True),
        # k_mtrx_batch: fp32 reaches it only with bit 0 and no LDS route (12 qubits)
        Case("s-b1-n12-04", 12, "mtrx_1q_batch", ([0, 4], u2() + u2())),
        Case("s-b1-12-13", n, "mtrx_1q_batch", ([12, 13], u2() + u2())),  # _v; fp64 k_mtrx_batch
        Case("s-b1-lds", n, "mtrx_1q_batch", ([0, 3, 7, 1, 10], sum((u2() for _ in range(5)), []))),
        Case("s-m2q-2-9", n, "mtrx_2q", (_clist(_unitary(rng, 4), precision), 9, 2)),
        Case("s-m2qb-pair2", n, "mtrx_2q_batch",
             (_clist([_unitary(rng, 4), _unitary(rng, 4)], precision), [12, 3], [0, 13])),
        Case("s-m2qb-lds", n, "mtrx_2q_batch",
             (_clist([_unitary(rng, 4) for _ in low], precision),
              [p[0] for p in low], [p[1] for p in low])),
        Case("s-fsimb-lds", n, "fsim_batch", (th, ph, [p[0] for p in low], [p[1] for p in low])),
        Case("s-cphase", n, "cphase_pairs", ([0, 5, 13], [7, 1, 2], [0.5, -1.25, 2.0]),
             native_sincos=True),
        Case("s-cnb-bit0", n, "cnot_batch", ([0, 9], [13, 4]), exact=True),   # k_cnot_batch
        Case("s-cnb-v", n, "cnot_batch", ([1, 13], [7, 4]), exact=True),      # k_cnot_batch_v
        Case("s-x_mask", n, "x_mask", (0b10010000100101,), exact=True),
        Case("s-phase_parity", n, "phase_parity", (th[0], 0b10010000100101)),
        Case("s-mux", n, "uniformly_controlled_single_bit",
             ([13, 0], 6, _round_c([_unitary(rng, 2) for _ in range(4)], precision).reshape(-1))),
    ]


STRIDE_CASES = {p: build_stride_cases(p) for p in PRECISIONS}


# ---- single-target cases for the QRACK_GPU_WIDE / _NT / _MFMA children (fp32) ---

def switch_cases(placements):
    """General, diagonal and antidiagonal uncontrolled gates at (n, target)."""
    out = []
    for n, t in placements:
        for kind in ("unitary", "diag", "antidiag"):
            out.append(_gate_case(f"sw{n}", n, kind, t, (), False, "fp32"))
    return out


WIDE_CASES = switch_cases([(10, 2), (10, 5), (10, 9), (3, 2), (10, 0), (10, 1), (14, 6)])
NT_CASES = switch_cases([(10, 0), (10, 1), (10, 9)])
MFMA_CASES = switch_cases([(3, 0), (3, 2), (10, 0), (10, 1), (10, 9)])


# ---- input, run, check -----------------------------------------------------------

def case_input(case, precision):
    """The case's input state, rounded to the engine's precision, as complex128."""
    state = go.random_state(case.n, _rng(case.id + "/state"))
    return state.astype(DTYPE[precision]).astype(np.complex128)


def case_expected(case, state):
    st = go.State(state)
    getattr(st, case.op)(*case.args)
    return st


def apply_case(sim, case, state, precision):
    sim.set_state_vector(state.astype(DTYPE[precision]))
    getattr(sim, case.op)(*case.args)
    return np.asarray(sim.get_state_vector())


def check_result(got, st, precision, case, c=3.0, sincos_rel_tol=None):
    """`got` against the oracle state `st` (see the module docstring).
    `sincos_rel_tol`, when given, replaces the derived bound for cases
    flagged native_sincos by |got - exp| <= tol |exp|."""
    got = np.asarray(got)
    assert got.dtype == DTYPE[precision]
    eps = EPS[precision]
    gates = max(st.gates, 1)
    if case.exact:
        want = st.v.astype(DTYPE[precision])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (
            f"{case.id}: {bad.size} amplitudes differ from the oracle; first at {bad[0]}: "
            f"got {got[bad[0]]!r}, expected {want[bad[0]]!r}")
        return 0.0
    got = got.astype(np.complex128)
    err = np.abs(got - st.v)
    norm2 = float(np.sum(np.abs(got) ** 2))
    if sincos_rel_tol is not None and case.native_sincos:
        ratio = float((err / np.abs(st.v)).max())
        print(f"{case.id}/{precision}: max |got - exp| / |exp| = {ratio:.3e} = {ratio / eps:.2f} eps")
        assert ratio <= sincos_rel_tol, f"{case.id}: {ratio:.3e} > {sincos_rel_tol:.3e}"
    else:
        if case.op in ANGLE_OPS:
            c += 1.0
        ratio = float((err / (gates * eps * st.a)).max())
        print(f"{case.id}/{precision}: G = {gates}, max err / (G eps a) = {ratio:.3f} (bound {c})")
        assert ratio <= c, f"{case.id}: error {ratio:.3f} G eps a exceeds {c} G eps a"
    print(f"{case.id}/{precision}: norm^2 - 1 = {norm2 - 1.0:.3e}")
    assert abs(norm2 - 1.0) <= 8 * gates * eps, f"{case.id}: norm^2 = {norm2!r}"
    return ratio


def run_case(sim, case, precision, **kw):
    state = case_input(case, precision)
    got = apply_case(sim, case, state, precision)
    return check_result(got, case_expected(case, state), precision, case, **kw)
