"""Lazy basis state, synthesised first QFT pass and cached sampling norms
of the HIP engine.

set_permutation only records "the state is phase*|perm>"; a QFT/IQFT whose
first pass is one of the two LDS kernels synthesises that state instead of
reading it, every other access materialises it first, and the forward low
ladder leaves per-tile norms that the sampler adds up instead of re-reading
the state. QRACK_GPU_QFT_LAZYPERM=0 / QRACK_GPU_QFT_SUMS=0 restore the
eager behaviour; they are read once per process, so every switch-off
comparison runs in a fresh child process that writes under tmp_path.
"""
import cmath
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
from ref_sim import assert_states_close

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = (1 + 0j, cmath.exp(0.7j))

# (name, precision, engine width, op, length) — which first pass each one
# selects is noted next to it
FIRST_PASS_CASES = (
    ("f32_n12", "fp32", 12, "qft", 12),  # low ladder, HBM-direct first group
    ("f32_n14", "fp32", 14, "qft", 14),  # mid, K=2
    ("f32_n16", "fp32", 16, "qft", 16),  # mid, K=4
    ("f32_n17", "fp32", 17, "qft", 17),  # trailing 5 -> 6-column pass below the tile
    ("f32_n18", "fp32", 18, "qft", 18),  # mid, two K=3 groups
    ("f32_n13", "fp32", 13, "qft", 13),  # first pass columnK -> materialise
    ("f32_e12_l8", "fp32", 12, "qft", 8),  # low ladder, copyIn
    ("f32_e12_l4", "fp32", 12, "qft", 4),  # low ladder, copyIn, one group
    ("f64_e11_l9", "fp64", 11, "qft", 9),
    ("f64_e11_l6", "fp64", 11, "qft", 6),
    ("f64_e11_l3", "fp64", 11, "qft", 3),
    ("f64_n12", "fp64", 12, "qft", 12),  # materialise, peeled column2, ladder
    ("f32_n12_inv", "fp32", 12, "iqft", 12),  # low ladder first
    ("f32_n16_inv", "fp32", 16, "iqft", 16),  # low ladder first, then mid
    ("f64_e11_l9_inv", "fp64", 11, "iqft", 9),  # low ladder first
    ("f32_n10_inv", "fp32", 10, "iqft", 10),  # below the tile: columnK -> materialise
)


def perms_for(width):
    mask = (1 << width) - 1
    return (0, mask, 0x5A5A5A5A & mask, 1 << (width - 1), 1)


_CHILD = r"""
import json, sys
mode, root, out = sys.argv[1], sys.argv[2], sys.argv[3]
if mode == "dlpack":
    import torch
    torch.cuda.init()  # torch first, engine second
sys.path.insert(0, root)
import numpy as np
import qrack_amd as qa

if mode == "first_pass":
    cases = json.loads(sys.argv[4])
    res = {}
    for name, prec, width, op, length, perms, phases in cases:
        for pi, perm in enumerate(perms):
            for fi, (re, im) in enumerate(phases):
                q = qa.create_simulator(width, engine="hip", precision=prec, seed=1)
                q.set_permutation(perm, complex(re, im))
                getattr(q, op)(0, length)
                res["%s__%d__%d" % (name, pi, fi)] = np.asarray(q.get_state_vector())
    np.savez(out, **res)
elif mode == "sums":
    res = {}
    for prec, n in (("fp32", 23), ("fp32", 24), ("fp64", 22), ("fp32", 14)):
        pows = [1 << i for i in range(n)]
        q = qa.create_simulator(n, engine="hip", precision=prec, seed=7)
        q.set_permutation(0x5A5A5A5A & ((1 << n) - 1))
        q.qft(0, n)
        uni = q.multi_shot_measure_mask(pows, 64)
        # a non-uniform distribution as well: superpose before the transform
        q.set_permutation(5)
        for i in range(0, n, 4):
            q.ry(0.9 + 0.05 * i, i)
        q.qft(0, n)
        skew = q.multi_shot_measure_mask(pows, 64)
        res["%s_%d" % (prec, n)] = [sorted(uni.items()), sorted(skew.items())]
    json.dump(res, open(out, "w"))
elif mode == "dlpack":
    res = {}
    # materialisation through the view
    n, p = 10, 0x2A5
    q = qa.create_simulator(n, engine="hip", seed=3)
    q.set_permutation(p)
    t = torch.from_dlpack(q.dlpack_view(0, 1 << n))
    res["view"] = t.cpu().numpy().tolist() == [1 if i == p else 0 for i in range(1 << n)]
    # invalidation: overwrite the transformed state with a basis state
    n, p = 23, 0x2B3C4D
    q = qa.create_simulator(n, engine="hip", seed=3)
    q.set_permutation(77)
    q.qft(0, n)
    t = torch.from_dlpack(q.dlpack_view(0, 1 << n))
    t.zero_()
    t[p] = 1
    torch.cuda.synchronize()
    shots = q.multi_shot_measure_mask([1 << i for i in range(n)], 32)
    res["shots"] = sorted(shots.items())
    res["want"] = [[p, 32]]
    json.dump(res, open(out, "w"))
print("CHILD_OK")
"""


def run_child(mode, out, env_extra, *extra):
    env = {**os.environ, **env_extra}
    r = subprocess.run(
        [sys.executable, "-c", _CHILD, mode, ROOT, str(out), *extra],
        env=env, capture_output=True, text=True, timeout=300,
    )
    assert "CHILD_OK" in r.stdout, f"stdout={r.stdout}\nstderr={r.stderr}"


def _case_payload():
    return json.dumps([
        [name, prec, width, op, length, list(perms_for(width)),
         [[ph.real, ph.imag] for ph in PHASES]]
        for name, prec, width, op, length in FIRST_PASS_CASES
    ])


@pytest.fixture(scope="module")
def first_pass_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("first_pass")
    payload = _case_payload()
    run_child("first_pass", d / "lazy.npz", {"QRACK_GPU_QFT_LAZYPERM": "1"}, payload)
    run_child("first_pass", d / "eager.npz", {"QRACK_GPU_QFT_LAZYPERM": "0"}, payload)
    return np.load(d / "lazy.npz"), np.load(d / "eager.npz")


@pytest.mark.parametrize("case", FIRST_PASS_CASES, ids=[c[0] for c in FIRST_PASS_CASES])
def test_first_pass_from_basis_state(first_pass_runs, case):
    """Bit-equal to the eager run of the same build (which also pins the
    global phase), and equal to the CPU engine within the tolerance of the
    existing QFT GPU tests."""
    lazy, eager = first_pass_runs
    name, prec, width, op, length = case
    tol = 2e-4 if prec == "fp32" else 1e-9
    for pi, perm in enumerate(perms_for(width)):
        for fi, phase in enumerate(PHASES):
            key = "%s__%d__%d" % (name, pi, fi)
            got, ref = lazy[key], eager[key]
            assert got.dtype == ref.dtype and got.shape == ref.shape
            assert got.tobytes() == ref.tobytes(), f"{key}: not bit-equal to the eager run"
            cp = qa.create_simulator(width, engine="cpu", precision=prec, seed=1)
            cp.set_permutation(perm, phase)
            getattr(cp, op)(0, length)
            want = np.asarray(cp.get_state_vector())
            assert_states_close(got, want, tol)


# ---- materialisation ---------------------------------------------------------

N_MAT = 10
P_MAT = 0x2A5


def basis(n, p, phase=1.0, dtype=np.complex64):
    v = np.zeros(1 << n, dtype=dtype)
    v[p] = phase
    return v


def pending(phase=1 + 0j, p=P_MAT, n=N_MAT):
    q = qa.create_simulator(n, engine="hip", seed=11)
    q.h(1)  # leave something else in the buffer first
    q.set_permutation(p, phase)
    return q


@pytest.mark.parametrize("phase", PHASES, ids=["phase1", "phase_e07"])
def test_materialise_amplitude_page(phase):
    page = np.asarray(pending(phase).get_amplitude_page(0, 1 << N_MAT))
    assert np.array_equal(page, basis(N_MAT, P_MAT, np.complex64(phase)))


def test_materialise_prob():
    for b in range(N_MAT):
        assert pending().prob(b) == float((P_MAT >> b) & 1)


def test_materialise_gate():
    q = pending(PHASES[1])
    q.h(0)
    cp = qa.create_simulator(N_MAT, engine="cpu", seed=11)
    cp.set_permutation(P_MAT, PHASES[1])
    cp.h(0)
    got = np.asarray(q.get_state_vector())
    want = np.asarray(cp.get_state_vector())
    assert np.count_nonzero(got) == 2
    assert np.allclose(got, want, atol=1e-6)


def test_materialise_second_set_permutation():
    q = pending()
    q.set_permutation(3)
    assert np.array_equal(np.asarray(q.get_state_vector()), basis(N_MAT, 3))


def test_materialise_compose():
    # pending on both sides of the compose
    q = pending()
    o = qa.create_simulator(2, engine="hip", seed=12)
    o.set_permutation(2)
    q.compose(o)
    assert np.array_equal(
        np.asarray(q.get_state_vector()), basis(N_MAT + 2, P_MAT | (2 << N_MAT)))


def test_materialise_clone():
    q = pending(PHASES[1])
    c = q.clone()
    want = basis(N_MAT, P_MAT, np.complex64(PHASES[1]))
    assert np.array_equal(np.asarray(c.get_state_vector()), want)
    assert np.array_equal(np.asarray(q.get_state_vector()), want)


def test_materialise_serialise_and_load(tmp_path):
    # unrotated int16 blocks keep the zeros exact; the one amplitude comes
    # back through a 16-bit quantiser and a normalisation, hence 1e-4
    path = str(tmp_path / "basis.qtq")
    qa.lossy_save_F(pending(), path, 4, 16, False)
    q2 = qa.create_simulator(N_MAT, engine="hip", seed=13)
    q2.set_permutation(1)  # pending in the engine that is loaded into, too
    qa.lossy_load_F(q2, path)
    got = np.asarray(q2.get_state_vector())
    assert abs(got[P_MAT] - 1) < 1e-4
    got[P_MAT] = 0
    assert not got.any()


def test_materialise_m_all():
    q = pending()
    assert q.m_all() == P_MAT
    assert np.array_equal(np.asarray(q.get_state_vector()), basis(N_MAT, P_MAT))


def test_fresh_engine_reads_back_initial_permutation():
    for prec, dt in (("fp32", np.complex64), ("fp64", np.complex128)):
        q = qa.create_simulator(N_MAT, engine="hip", precision=prec, init_perm=P_MAT, seed=2)
        sv = np.asarray(q.get_state_vector())
        assert np.array_equal(np.abs(sv), np.abs(basis(N_MAT, P_MAT, dtype=dt)))
        assert abs(abs(sv[P_MAT]) - 1) < 1e-6


# ---- cached norms ------------------------------------------------------------


@pytest.fixture(scope="module")
def sums_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sums")
    run_child("sums", d / "on.json", {"QRACK_GPU_QFT_SUMS": "1"})
    run_child("sums", d / "off.json", {"QRACK_GPU_QFT_SUMS": "0"})
    return json.load(open(d / "on.json")), json.load(open(d / "off.json"))


@pytest.mark.parametrize("key", ["fp32_23", "fp32_24", "fp64_22"])
def test_sampling_from_tile_sums_matches_state_sums(sums_runs, key):
    on, off = sums_runs
    assert on[key] == off[key]
    assert sum(c for _, c in on[key][0]) == 64 and sum(c for _, c in on[key][1]) == 64


def test_sampling_below_tile_size_falls_back(sums_runs):
    # n = 14: a sampling chunk (8 amplitudes) is smaller than a tile
    on, off = sums_runs
    assert on["fp32_14"] == off["fp32_14"]


N_INV = 23
POWS_INV = [1 << i for i in range(N_INV)]


def transformed(p0):
    q = qa.create_simulator(N_INV, engine="hip", seed=21)
    q.set_permutation(p0)
    q.qft(0, N_INV)  # tile sums valid from here
    return q


def test_sums_dropped_by_iqft():
    q = transformed(0x31C5A7)
    q.iqft(0, N_INV)
    assert q.multi_shot_measure_mask(POWS_INV, 32) == {0x31C5A7: 32}


def test_sums_dropped_by_set_permutation():
    q = transformed(0x31C5A7)
    q.set_permutation(0x5B0F12)
    assert q.multi_shot_measure_mask(POWS_INV, 32) == {0x5B0F12: 32}


def test_sums_dropped_by_gate_then_iqft():
    # QFT|0> is uniform, X(0) maps it onto itself, IQFT brings back |0>
    q = transformed(0)
    q.x(0)
    q.iqft(0, N_INV)
    assert q.multi_shot_measure_mask(POWS_INV, 32) == {0: 32}


def test_dlpack_view_materialises_and_drops_sums(tmp_path):
    out = tmp_path / "dlpack.json"
    run_child("dlpack", out, {})
    res = json.load(open(out))
    assert res["view"] is True
    assert res["shots"] == res["want"]
