"""pauli_rotation and evolve_pauli_sum: the planner, the CPU engine's one-pass
path, the default lowering through the layers, validation, the C ABI and the
example.

Oracle and bounds: pauli_evolve_oracle (numpy float64, per-term factors in
the defined order). Inputs are random dense states set with set_state_vector
and read back, so the oracle starts from exactly the engine's amplitudes.
Every case keeps |tau| sum|coeff| of one X/Y mask at or below 1.
"""
import ctypes
import glob
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po
import pauli_evolve_oracle as peo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("fp32", "fp64")
WIDTHS = (1, 2, 3, 5, 9)
STATE_TOL = 1e-5  # the CPU suite's state tolerance (ref_sim.assert_states_close)


def engine_with_state(n, prec, seed, **kw):
    rng = np.random.default_rng(seed)
    kw.setdefault("engine", "cpu")
    q = qa.create_simulator(n, precision=prec, seed=1, **kw)
    q.set_state_vector(po.random_state(n, rng, peo.DTYPE[prec]))
    return q, np.asarray(q.get_state_vector()), rng


def heisenberg(n, jx=1.0, jy=0.8, jz=0.6):
    terms = []
    for b in range(n - 1):
        terms += [(jx, [b, b + 1], [1, 1]), (jy, [b, b + 1], [3, 3]), (jz, [b, b + 1], [2, 2])]
    return terms


def scaled_time(terms, steps=1):
    """a time that puts the heaviest X/Y mask exactly at the oracle's load limit"""
    return steps / peo.group_load(terms, 1.0)


# ---- 1. the CPU engine against the oracle ----------------------------------------


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", WIDTHS)
def test_rotations_match_oracle(n, prec):
    q, sv, rng = engine_with_state(n, prec, 500 + n)
    if n <= 3:
        strings = [(list(range(n)), list(ps)) for ps in itertools.product(range(4), repeat=n)]
    else:
        strings = [po.random_string(n, rng) for _ in range(48)]
    for k, (qs, ps) in enumerate(strings):
        theta = float(rng.uniform(-1, 1))
        q.set_state_vector(sv)
        q.pauli_rotation(qs, ps, theta)
        want, a, gates = peo.rotate(sv, qs, ps, theta)
        peo.check(q.get_state_vector(), want, a, gates, prec, f"n{n} {qs} {ps}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("n", WIDTHS)
def test_sums_match_oracle(n, order, prec):
    q, sv, rng = engine_with_state(n, prec, 600 + n)
    terms = po.random_terms(n, rng, 30) + [(0.4, [], [])]
    steps = 3
    time = scaled_time(terms, steps)
    assert peo.group_load(terms, time, steps) <= 1.0 + 1e-12
    q.evolve_pauli_sum(terms, time, steps, order)
    want, a, gates = peo.evolve(sv, terms, time, steps, order)
    peo.check(q.get_state_vector(), want, a, gates, prec, f"n{n} order{order}")


def test_z_rotation_is_rz_of_twice_the_angle():
    a, sv, _ = engine_with_state(3, "fp64", 11)
    b, _, _ = engine_with_state(3, "fp64", 11)
    a.pauli_rotation([1], [2], 0.37)
    b.rz(0.74, 1)
    assert np.abs(np.asarray(a.get_state_vector()) - np.asarray(b.get_state_vector())).max() < 1e-15


def test_identity_string_is_a_global_phase():
    q, sv, _ = engine_with_state(3, "fp64", 12)
    q.pauli_rotation([], [], 0.3)
    q.pauli_rotation([2, 0], [0, 0], 0.2)
    assert np.abs(np.asarray(q.get_state_vector()) - np.exp(-0.5j) * sv).max() < 1e-15


# ---- 2. the planner ----------------------------------------------------------------


def test_plan_heisenberg_first_order():
    """All ZZ terms share x = 0 and XX, YY of a bond share its x: 1 + 5 passes."""
    plan = qa.pauli_evolve_plan(heisenberg(6), 6, 0.1, 1, 1)
    assert len(plan) == 6
    assert [x for _, x, _ in plan] == [0] + sorted(3 << b for b in range(5))
    assert [g for g, _, _ in plan] == list(range(6))
    for _, _, segs in plan:
        assert [(s, pytest.approx(t)) for s, t in segs] == [("re", 0.1)]


def test_plan_heisenberg_second_order_merges():
    """A second-order step walks the 6 groups forth and back: 12 passes, of
    which the two on the last group are adjacent and merge, 11. Across each of
    the steps - 1 step boundaries the two passes on group 0 merge as well:
    3 * 11 - 2 = 31. Merged angles add."""
    steps, time = 3, 0.3
    plan = qa.pauli_evolve_plan(heisenberg(6), 6, time, steps, 2)
    assert len(plan) == 3 * 11 - 2 == 31
    groups = [g for g, _, _ in plan]
    assert all(p != q for p, q in zip(groups, groups[1:]))
    tau = time / steps
    for k, (g, _, segs) in enumerate(plan):
        assert len(segs) == 1 and segs[0][0] == "re"
        merged = g == 5 or (g == 0 and 0 < k < len(plan) - 1)
        assert segs[0][1] == pytest.approx(tau if merged else tau / 2)
    # every group is turned by `time` in total
    for g in range(6):
        assert sum(segs[0][1] for gg, _, segs in plan if gg == g) == pytest.approx(time)


def test_plan_mixed_group_keeps_the_order_of_its_sets():
    """X0X1 (re) and X0Y1 (im) share x and do not commute: a merged pass keeps
    them as alternating segments and only adds angles of the same set."""
    terms = [(1.0, [0, 1], [1, 1]), (1.0, [0, 1], [1, 3])]
    plan = qa.pauli_evolve_plan(terms, 2, 0.2, 1, 2)
    assert len(plan) == 1
    assert [(s, pytest.approx(t)) for s, t in plan[0][2]] == [("re", 0.1), ("im", 0.2), ("re", 0.1)]
    assert len(qa.pauli_evolve_plan(terms, 2, 0.2, 1, 1)[0][2]) == 2


def test_plan_identities_only():
    assert qa.pauli_evolve_plan([(0.7, [], []), (0.2, [1], [0])], 3, 0.5, 2, 2) == []
    for prec in PRECS:
        q, sv, _ = engine_with_state(3, prec, 13)
        q.evolve_pauli_sum([(0.7, [], []), (0.2, [1], [0])], 0.5, 2, 2)
        want, a, gates = peo.evolve(sv, [(0.9, [], [])], 0.5)
        assert gates == 1
        peo.check(q.get_state_vector(), want, a, gates, prec, "identities")


def test_plan_rejects_bad_arguments():
    t = heisenberg(3)
    for steps, order in ((0, 1), (-1, 2), (1, 0), (1, 3)):
        with pytest.raises(Exception):
            qa.pauli_evolve_plan(t, 3, 0.1, steps, order)
    with pytest.raises(Exception):
        qa.pauli_evolve_plan([(1.0, [3], [1])], 3, 0.1, 1, 1)


# ---- 3. default lowering through the layers ----------------------------------------

LAYERS = [
    dict(layers=["qunit", "cpu"]),
    dict(layers=["stabilizer_hybrid", "cpu"]),
    dict(layers=["pager", "cpu"]),
    dict(engine="sparse"),
]


def entangle(q, n):
    for i in range(n):
        q.h(i)
        q.ry(0.2 + 0.3 * i, i)
    for i in range(n - 1):
        q.cnot(i, i + 1)
    for i in range(n):
        q.rz(0.15 * (i + 1), i)


# X0X1 and X0Y1 share x and anticommute: the product of their two rotations at
# tau = 0.5 differs from exp(-i tau (X0X1 + X0Y1)) by about tau^2 = 0.25
NONCOMMUTING = [(1.0, [0, 1], [1, 1]), (1.0, [0, 1], [1, 3])]


@pytest.mark.parametrize("kw", LAYERS, ids=lambda kw: "-".join(kw.get("layers", [kw.get("engine")])))
@pytest.mark.parametrize("order", (1, 2))
def test_default_lowering_matches_oracle(kw, order):
    n = 6
    rng = np.random.default_rng(41)
    sums = {
        "heisenberg": (heisenberg(n) + [(0.3, [], [])], 0.4, 2),
        "random": (po.random_terms(n, rng, 12), 0.3, 2),
        "noncommuting": (NONCOMMUTING + heisenberg(n), 0.5, 1),
    }
    for name, (terms, time, steps) in sums.items():
        q = qa.create_simulator(n, seed=3, **kw)
        entangle(q, n)
        before = np.asarray(q.get_state_vector())
        q.evolve_pauli_sum(terms, time, steps, order)
        want, _, _ = peo.evolve(before, terms, time, steps, order)
        got = np.asarray(q.get_state_vector())
        assert np.abs(got - want).max() <= STATE_TOL, (name, np.abs(got - want).max())


def test_noncommuting_pair_is_not_exponentiated_as_a_sum():
    """The margin of the case above: the defined product and the exact
    exponential of the group's sum differ by far more than 1e-3, and the CPU
    engine's one-pass form gives the product."""
    tau = 0.5
    q, sv, _ = engine_with_state(2, "fp64", 14)
    want, a, gates = peo.evolve(sv, NONCOMMUTING, tau)
    h = np.zeros((4, 4), dtype=complex)
    for c, qs, ps in NONCOMMUTING:
        x, z, ny = po.masks(qs, ps)
        for k in range(4):
            h[k ^ x, k] += c * 1j ** (ny % 4) * (-1) ** bin(k & z).count("1")
    assert np.allclose(h, h.conj().T)
    w, v = np.linalg.eigh(h)
    exact = (v * np.exp(-1j * tau * w)) @ v.conj().T @ sv
    assert np.abs(exact - want).max() > 1e-3
    q.evolve_pauli_sum(NONCOMMUTING, tau)
    peo.check(q.get_state_vector(), want, a, gates, "fp64", "noncommuting")


@pytest.mark.parametrize("kw", LAYERS, ids=lambda kw: "-".join(kw.get("layers", [kw.get("engine")])))
def test_default_rotation_matches_oracle(kw):
    n = 6
    rng = np.random.default_rng(42)
    q = qa.create_simulator(n, seed=3, **kw)
    entangle(q, n)
    strings = [([], []), ([2], [2]), ([1, 4], [0, 0]), ([0, 5], [3, 1])]
    strings += [po.random_string(n, rng) for _ in range(8)]
    for qs, ps in strings:
        theta = float(rng.uniform(-1, 1))
        before = np.asarray(q.get_state_vector())
        q.pauli_rotation(qs, ps, theta)
        want, _, _ = peo.rotate(before, qs, ps, theta)
        got = np.asarray(q.get_state_vector())
        assert np.abs(got - want).max() <= STATE_TOL, (qs, ps, np.abs(got - want).max())


@pytest.mark.parametrize("layers", (["fuser", "cpu"], ["hybrid"]), ids=lambda l: "-".join(l))
def test_wrappers_forward(layers):
    n = 6
    terms = heisenberg(n)
    bare = qa.create_simulator(n, engine="cpu", seed=3)
    q = qa.create_simulator(n, layers=layers, seed=3)
    for s in (bare, q):
        entangle(s, n)
        s.evolve_pauli_sum(terms, 0.4, 2, 2)
        s.pauli_rotation([0, 3], [3, 1], 0.3)
    d = np.abs(np.asarray(q.get_state_vector()) - np.asarray(bare.get_state_vector())).max()
    assert d <= STATE_TOL


# ---- 4. validation -------------------------------------------------------------------


@pytest.mark.parametrize("kw", [dict(engine="cpu")] + LAYERS[:1],
                         ids=lambda kw: "-".join(kw.get("layers", [kw.get("engine")])))
def test_argument_errors_throw(kw):
    n = 4
    q = qa.create_simulator(n, seed=1, **kw)
    for qs, ps in (([0, 1], [1]), ([0], [4]), ([n], [1]), ([1, 1], [1, 2])):
        with pytest.raises(Exception):
            q.pauli_rotation(qs, ps, 0.1)
        with pytest.raises(Exception):
            q.evolve_pauli_sum([(1.0, qs, ps)], 0.1)
    ok = [(1.0, [0, 1], [1, 1])]
    for steps, order in ((0, 1), (-2, 1), (1, 0), (1, 3)):
        with pytest.raises(Exception):
            q.evolve_pauli_sum(ok, 0.1, steps, order)
    # nothing above touched the state
    assert abs(q.prob_all(0) - 1.0) < 1e-6


# ---- 5. the C ABI ----------------------------------------------------------------------


def test_capi_agrees_with_python():
    so = glob.glob(os.path.join(REPO, "qrack_amd", "_qrack*.so"))[0]
    lib = ctypes.CDLL(so)
    lib.qrack_init_count_type.restype = ctypes.c_uint64
    lib.qrack_prob.restype = ctypes.c_double
    lib.qrack_expectation_pauli_sum.restype = ctypes.c_double
    lib.qrack_pauli_rotation.restype = None
    lib.qrack_evolve_pauli_sum.restype = None
    u64, dbl = ctypes.c_uint64, ctypes.c_double
    n = 3
    terms = heisenberg(n) + [(0.25, [], [])]
    coeffs = (dbl * len(terms))(*[c for c, _, _ in terms])
    lens = (u64 * len(terms))(*[len(qs) for _, qs, _ in terms])
    flat_q = [b for _, qs, _ in terms for b in qs]
    flat_p = [p for _, _, ps in terms for p in ps]
    qs_c = (u64 * len(flat_q))(*flat_q)
    ps_c = (ctypes.c_int * len(flat_p))(*flat_p)

    sid = lib.qrack_init_count_type(n, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert sid != 0
    q = qa.create_simulator(n, engine="cpu", seed=1)
    lib.qrack_h(u64(sid), u64(0))
    q.h(0)
    lib.qrack_pauli_rotation(u64(sid), (ctypes.c_int * 2)(3, 1), (u64 * 2)(0, 2), u64(2), dbl(0.3))
    q.pauli_rotation([0, 2], [3, 1], 0.3)
    lib.qrack_evolve_pauli_sum(u64(sid), u64(len(terms)), coeffs, lens, qs_c, ps_c, dbl(0.7),
                               ctypes.c_int(2), ctypes.c_int(2))
    q.evolve_pauli_sum(terms, 0.7, 2, 2)
    assert lib.qrack_get_error(u64(sid)) == 0
    for b in range(n):
        assert abs(lib.qrack_prob(u64(sid), u64(b)) - q.prob(b)) <= 1e-5
    probe = [(1.0, [0, 1], [1, 3]), (0.5, [1, 2], [3, 2]), (0.25, [0], [1])]
    pc = (dbl * 3)(1.0, 0.5, 0.25)
    pl = (u64 * 3)(2, 2, 1)
    pq = (u64 * 5)(0, 1, 1, 2, 0)
    pp = (ctypes.c_int * 5)(1, 3, 3, 2, 1)
    e = lib.qrack_expectation_pauli_sum(u64(sid), u64(3), pc, pl, pq, pp)
    assert abs(e - q.expectation_pauli_sum(probe)) <= 1e-5
    # argument errors are reported through the error flag, not a crash
    lib.qrack_pauli_rotation(u64(sid), (ctypes.c_int * 2)(1, 2), (u64 * 2)(1, 1), u64(2), dbl(0.1))
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))
    sid = lib.qrack_init_count_type(n, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    lib.qrack_evolve_pauli_sum(u64(sid), u64(len(terms)), coeffs, lens, qs_c, ps_c, dbl(0.7),
                               ctypes.c_int(1), ctypes.c_int(3))
    assert lib.qrack_get_error(u64(sid)) != 0
    lib.qrack_destroy(u64(sid))


# ---- 6. the example --------------------------------------------------------------------


def test_example_runs():
    out = subprocess.run(
        [sys.executable, "pauli_sum_evolve.py", "--engine", "cpu", "--qubits", "8"],
        cwd=os.path.join(REPO, "examples"), capture_output=True, text=True, timeout=300,
        env={**os.environ, "PYTHONPATH": REPO},
    )
    assert out.returncode == 0, f"{out.stdout}\n{out.stderr}"
    assert "OK" in out.stdout
