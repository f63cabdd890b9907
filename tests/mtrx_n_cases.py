"""Case table, input builder and checks shared by test_mtrx_n_cpu.py and
test_mtrx_n_gpu.py: mtrx_n(qubits, matrix, controls, anti) against
gate_oracle.State.apply, which already is the oracle for this call.

Input: gate_cases.case_input (a fixed-seed complex Gaussian state rounded to
the engine's dtype), or a basis state set with set_permutation where the case
says so. Matrices are rounded to the engine's dtype before either side sees
them.

Tolerance (derived, not measured), elementwise:

    |got_i - exp_i| <= c(k) * G * eps_R * a_i,   c(k) = max(3, ceil((sqrt(5) + 2^k - 1) / 2))

G is the number of matrices the oracle applied and a_i its companion vector
(|v| pushed through |M|). To first order, with u = eps/2, one complex multiply
is off by at most sqrt(5) u of its magnitude and a 2^k-term sum adds
(2^k - 1) u in any summation order, so a row of a 2^k x 2^k costs
(sqrt(5) + 2^k - 1) / 2 eps of a_i: 3, 3, 5, 9, 17, 33 for k = 1..6, where
k = 1 and 2 keep the 3 of gate_cases (it also covers the MFMA form of a 2x2).
Where a_i = 0 every partial sum is zero and the amplitude must be exactly 0.

Unitary cases also assert

    | ||got||^2 - ||exp||^2 | <= 2 t S1 + t^2 S2,   t = c(k) G eps,
    S1 = sum |exp_i| a_i,   S2 = sum a_i^2

which follows from the elementwise bound with nothing fitted: with
got_i = exp_i + d_i and |d_i| <= t a_i, | |got_i|^2 - |exp_i|^2 | <=
2 |exp_i| |d_i| + |d_i|^2.

Exact cases (identity, a basis permutation) only move amplitudes and are
compared with np.array_equal. In controlled cases the amplitudes outside the
control subspace are compared with np.array_equal against the input.
"""

import math
from typing import NamedTuple, Optional

import numpy as np

import gate_oracle as go
from gate_cases import DTYPE, EPS, _clist, _rng, _unitary, case_input

PRECISIONS = ("fp32", "fp64")
MTRXN_MAX = 6
KINDS = ("haar", "identity", "shift", "diag", "gauss")


def c_of_k(k):
    return max(3, math.ceil((math.sqrt(5.0) + 2**k - 1) / 2))


assert [c_of_k(k) for k in range(1, 7)] == [3, 3, 5, 9, 17, 33]


class Case(NamedTuple):
    id: str
    n: int
    qubits: tuple
    controls: tuple = ()
    anti: bool = False
    kind: str = "haar"
    perm: Optional[int] = None  # start from set_permutation(perm)

    @property
    def k(self):
        return len(self.qubits)

    @property
    def exact(self):
        return self.kind in ("identity", "shift")

    @property
    def unitary(self):
        return self.kind != "gauss"


def case_matrix(case, precision):
    """The case's matrix as a flat list of complex, rounded to `precision`."""
    rng = _rng(case.id + "/matrix")
    d = 1 << case.k
    if case.kind == "haar":
        m = _unitary(rng, d)
    elif case.kind == "identity":
        m = np.eye(d)
    elif case.kind == "shift":  # |s> -> |s + 1 mod d>
        m = np.roll(np.eye(d), 1, axis=0)
    elif case.kind == "diag":
        m = np.diag(np.exp(1j * rng.uniform(0.3, 2 * np.pi - 0.3, d)))
    else:  # complex Gaussian, not unitary
        m = (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / math.sqrt(2 * d)
    return _clist(m, precision)


def _c(tag, n, qubits, controls=(), anti=False, kind="haar", perm=None):
    q = "_".join(map(str, qubits))
    cid = f"{tag}-n{n}-k{len(qubits)}-q{q}"
    if controls:
        cid += ("-a" if anti else "-c") + "_".join(map(str, controls))
    if kind != "haar":
        cid += "-" + kind
    if perm is not None:
        cid += f"-perm{perm}"
    return Case(cid, n, tuple(qubits), tuple(controls), anti, kind, perm)


def build_cases():
    out = []
    # one orbit, and two
    for k in range(1, 7):
        out.append(_c("full", k, range(k)))
    out += [_c("two", 7, (0, 1, 2, 3, 4, 5)), _c("two", 7, (6, 1, 2, 3, 4, 5))]
    # the state is smaller than the tile
    for qs in ((0, 1, 2), (7, 8, 9), (0, 5, 9), (9, 0, 5), (1, 3, 6, 8), (0, 2, 4, 7, 9),
               (0, 2, 4, 6, 8, 9)):
        out.append(_c("small", 10, qs))
    # 4 tiles (fp32) or 8 (fp64): all targets low, all in the top bits, straddling
    for qs in ((0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4, 5), (11, 12, 13), (10, 11, 12, 13),
               (8, 9, 10, 11, 12, 13), (0, 1, 6, 11, 12, 13), (5, 13, 2)):
        out.append(_c("tiles", 14, qs))
    # k = 1 and the uncontrolled k = 2 delegate
    out += [_c("route", 10, (4,)), _c("route", 10, (7, 2)), _c("route", 14, (13,), (0,)),
            _c("route", 14, (12,), (3, 13), anti=True)]
    # controls: on bit 0 (inside the run), on the top bit, between targets,
    # and two of them (at 14 qubits one inside the tile and one outside)
    targets = {
        10: {2: (2, 5), 3: (1, 4, 8), 5: (1, 3, 5, 6, 8)},
        14: {2: (2, 5), 3: (1, 4, 9), 5: (1, 3, 6, 8, 10)},
    }
    between = {2: 3, 3: 6, 5: 4}
    for n in (10, 14):
        for k in (2, 3, 5):
            qs = targets[n][k]
            for cs in ((0,), (n - 1,), (between[k],), (7, n - 1)):
                for anti in (False, True):
                    out.append(_c("ctl", n, qs, cs, anti))
    # high targets with a control inside the run, and every control outside the tile
    out += [_c("ctl", 14, (11, 12, 13), (0,)), _c("ctl", 14, (11, 9, 10), (5, 13), anti=True),
            _c("ctl", 14, (0, 1, 2, 3), (12, 13)), _c("ctl", 14, (3, 2, 1, 0), (12, 13), anti=True)]
    # matrix kinds
    for n, qs in ((10, (0, 5, 9)), (14, (5, 13, 2)), (10, (1, 3, 6, 8)), (14, (0, 1, 6, 11, 12, 13))):
        for kind in ("identity", "diag", "gauss") + (("shift",) if len(qs) == 3 else ()):
            out.append(_c("kind", n, qs, kind=kind))
    out += [_c("kind", 14, (5, 13, 2), (0, 12), kind="shift"),
            _c("kind", 10, (1, 3, 6, 8), (0,), anti=True, kind="identity"),
            _c("kind", 14, (1, 3, 6, 8, 10), (13,), kind="gauss")]
    # from a basis state that is still pending on the HIP engine
    out += [_c("basis", 10, (2, 0, 7), perm=5), _c("basis", 10, (1, 3, 6, 8), (0,), perm=5)]
    return out


CASES = build_cases()
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)
BY_ID = {c.id: c for c in CASES}
# through the layers: k = 3 unsorted, k = 4 with a control, an anti-control
REDUCED = [_c("layer", 6, (4, 0, 2)), _c("layer", 6, (0, 1, 3, 5), (2,)),
           _c("layer", 6, (5, 1), (3, 0), anti=True)]


def route_of(case):
    """Profile op the HIP engine must show for the case."""
    if case.k == 1:
        return "apply2x2"
    if case.k == 2 and not case.controls:
        return "mtrx_2q"
    return "mtrx_n"


ROUTE_OPS = ("apply2x2", "mtrx_2q", "mtrx_n")


def input_state(case, precision):
    if case.perm is not None:
        v = np.zeros(1 << case.n, dtype=np.complex128)
        v[case.perm] = 1.0
        return v
    return case_input(case, precision)


def load_input(sim, case, precision):
    if case.perm is not None:
        sim.set_permutation(case.perm)
    else:
        sim.set_state_vector(input_state(case, precision).astype(DTYPE[precision]))


def apply_case(sim, case, precision):
    load_input(sim, case, precision)
    sim.mtrx_n(list(case.qubits), case_matrix(case, precision), list(case.controls), case.anti)
    return np.asarray(sim.get_state_vector())


def expected(case, precision):
    st = go.State(input_state(case, precision))
    st.apply(case.qubits, case_matrix(case, precision), case.controls, case.anti)
    return st


def check_state(got, st, precision, k, label, exact=False, unitary=True, c_sum=None):
    """`got` against the oracle state `st` (see the module docstring); returns
    the measured max err / (G eps a). `c_sum`, for a circuit of gates of
    several widths, is the sum of c over its gates and replaces c(k) G."""
    got = np.asarray(got)
    assert got.dtype == DTYPE[precision]
    if exact:
        want = st.v.astype(DTYPE[precision])
        assert np.array_equal(got, want), f"{label}: differs from the oracle"
        return 0.0
    eps = EPS[precision]
    gates = max(st.gates, 1)
    if c_sum is None:
        c_sum = c_of_k(k) * gates
    t = c_sum * eps
    got = got.astype(np.complex128)
    err = np.abs(got - st.v)
    zero = st.a == 0
    assert not np.any(err[zero]), f"{label}: amplitude with a_i = 0 is not 0"
    ratio = float((err[~zero] / (gates * eps * st.a[~zero])).max())
    bound = c_sum / gates
    print(f"{label}/{precision}: G = {gates}, max err / (G eps a) = {ratio:.3f} (bound {bound:g})")
    assert ratio <= bound, f"{label}: error {ratio:.3f} G eps a exceeds {bound:g} G eps a"
    if unitary:
        n_got, n_exp = float(np.sum(np.abs(got) ** 2)), float(np.sum(np.abs(st.v) ** 2))
        nb = 2 * t * float(np.sum(np.abs(st.v) * st.a)) + t * t * float(np.sum(st.a**2))
        print(f"{label}/{precision}: norm^2 difference {n_got - n_exp:.3e} (bound {nb:.3e})")
        assert abs(n_got - n_exp) <= nb, f"{label}: norm^2 = {n_got!r}, expected {n_exp!r}"
    return ratio


def check_case(got, case, precision):
    st = expected(case, precision)
    if case.controls:
        start = input_state(case, precision).astype(DTYPE[precision])
        idx = np.arange(1 << case.n)
        cmask = sum(1 << c for c in case.controls)
        off = (idx & cmask) != (0 if case.anti else cmask)
        assert np.array_equal(np.asarray(got)[off], start[off]), (
            f"{case.id}: amplitudes outside the control subspace changed")
    return check_state(got, st, precision, case.k, case.id, exact=case.exact, unitary=case.unitary)


def run_case(sim, case, precision):
    return check_case(apply_case(sim, case, precision), case, precision)
