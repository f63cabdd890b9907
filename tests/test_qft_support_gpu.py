"""Support-restricted QFT/IQFT of a lazy basis state on the HIP engine.

A full-width fp32 transform of phase*|p> whose plan holds only low and mid
passes runs every pass but the last on the few tiles that can hold a nonzero
amplitude, reads the buffer only inside that support and writes the whole
state once, in the last pass (qa.qft_support_plan gives the schedule).
QRACK_GPU_QFT_SUPPORT=0 restores the full sweeps. Every nonzero amplitude
goes through the same instructions either way, so the states must be equal
byte for byte. The switches are read once per process, so each setting runs
in its own child process.
"""
import cmath
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
PHASES = (1 + 0j, cmath.exp(0.7j))
TOL = 2e-4  # the fp32 tolerance of the existing QFT GPU tests
OPS = ("qft", "iqft")
WIDTHS = (14, 16, 17, 18, 20, 21, 22, 23, 25)
CPU_MAX_WIDTH = 21
# (engine width, register length) that must keep the unrestricted path: a
# register-column pass in the plan (19, 13), a register shorter than the engine
FALLBACKS = ((19, 19), (13, 13), (22, 21))
BIG = 28  # mid8@20, mid8@12, low12: the middle restricted pass is the wide kernel
ON = {"QRACK_GPU_QFT_SUPPORT": "1"}
OFF = {"QRACK_GPU_QFT_SUPPORT": "0"}


def perms_for(width):
    mask = (1 << width) - 1
    return (0, mask, 0x5A5A5A5A & mask, 1 << (width - 1), 1)


_CHILD = r"""
import hashlib, json, sys
root, tests, out, mode = sys.argv[1:5]
spec = json.loads(sys.argv[5])
if mode == "big":
    import torch
    torch.cuda.init()  # torch first, engine second
sys.path.insert(0, root)
sys.path.insert(0, tests)
import numpy as np
import qrack_amd as qa
from ref_sim import assert_states_close

res = {}
if mode == "states":
    for width, length, op, with_cpu, perms, phases in spec["cases"]:
        for pi, perm in enumerate(perms):
            for fi, (re, im) in enumerate(phases):
                q = qa.create_simulator(width, engine="hip", seed=1)
                q.set_permutation(perm, complex(re, im))
                getattr(q, op)(0, length)
                got = np.asarray(q.get_state_vector())
                r = {"sha": hashlib.sha256(got.tobytes()).hexdigest(), "close_err": None}
                if with_cpu:
                    cp = qa.create_simulator(width, engine="cpu", precision="fp64", seed=1)
                    cp.set_permutation(perm, complex(re, im))
                    getattr(cp, op)(0, length)
                    try:
                        assert_states_close(got, np.asarray(cp.get_state_vector()), spec["tol"])
                    except AssertionError as e:
                        r["close_err"] = str(e)
                res["%d_%d_%s_%d_%d" % (width, length, op, pi, fi)] = r
                del q
elif mode == "big":
    width = spec["width"]
    g = torch.Generator().manual_seed(20240229 + width)
    idx = torch.randint(0, 1 << width, (1 << 16,), generator=g).cuda()
    samples = {}
    for op in spec["ops"]:
        for pi, (perm, (re, im)) in enumerate(spec["inputs"]):
            q = qa.create_simulator(width, engine="hip", seed=1)
            q.set_permutation(perm, complex(re, im))
            getattr(q, op)(0, width)
            q.finish()
            t = torch.from_dlpack(q.dlpack_view(0, 1 << width))
            raw = torch.view_as_real(t).view(torch.int32)
            name = "%s_%d" % (op, pi)
            res[name] = {
                "bitsum": int(raw.sum(dtype=torch.int64).item()),
                "norm": float(torch.linalg.vector_norm(torch.view_as_real(t).double()).item()),
            }
            samples[name] = t[idx].cpu().numpy()
            del t, raw, q
    np.savez(out + ".npz", **samples)
elif mode == "shots":
    for n in spec["widths"]:
        pows = [1 << i for i in range(n)]
        for pi, perm in enumerate(spec["perms"]):
            q = qa.create_simulator(n, engine="hip", seed=7)
            q.set_permutation(perm & ((1 << n) - 1))
            q.qft(0, n)
            res["%d_%d" % (n, pi)] = sorted(q.multi_shot_measure_mask(pows, 64).items())
json.dump(res, open(out, "w"))
print("CHILD_OK")
"""


def run_child(out, env_extra, mode, spec):
    env = {**os.environ, **env_extra}
    r = subprocess.run(
        [sys.executable, "-c", _CHILD, ROOT, TESTS, str(out), mode, json.dumps(spec)],
        env=env, capture_output=True, text=True, timeout=600,
    )
    assert "CHILD_OK" in r.stdout, f"stdout={r.stdout[-2000:]}\nstderr={r.stderr[-4000:]}"
    return json.load(open(out))


def _phases():
    return [[ph.real, ph.imag] for ph in PHASES]


class _StateRuns:
    """Switch-on and switch-off runs of one engine shape, made when first
    asked for so every shape's test pays for its own: both ops in one pair of
    children, one pair per op from 23 qubits up, where copying out and
    hashing the states is what takes the time."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.cache = {}

    def get(self, width, length, op):
        ops = (op,) if width >= 23 else OPS
        key = (width, length, ops)
        if key not in self.cache:
            tag = "%d_%d_%s" % (width, length, "_".join(ops))
            with_cpu = width == length and width <= CPU_MAX_WIDTH
            spec = {"tol": TOL, "cases": [
                [width, length, o, with_cpu, list(perms_for(width)), _phases()] for o in ops]}
            on = run_child(self.tmp / ("on_%s.json" % tag), ON, "states", spec)
            spec["cases"] = [c[:3] + [False] + c[4:] for c in spec["cases"]]
            off = run_child(self.tmp / ("off_%s.json" % tag), OFF, "states", spec)
            self.cache[key] = (on, off)
        return self.cache[key]


@pytest.fixture(scope="module")
def state_runs(tmp_path_factory):
    return _StateRuns(tmp_path_factory.mktemp("support_states"))


def _compare(state_runs, width, length, op):
    on, off = state_runs.get(width, length, op)
    for pi in range(len(perms_for(width))):
        for fi in range(len(PHASES)):
            name = "%d_%d_%s_%d_%d" % (width, length, op, pi, fi)
            assert on[name]["sha"] == off[name]["sha"], f"{name}: differs from the switch-off run"
            assert on[name]["close_err"] is None, (name, on[name]["close_err"])


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("width", WIDTHS)
def test_bit_equal_to_the_unrestricted_run(state_runs, width, op):
    """Byte-equal to QRACK_GPU_QFT_SUPPORT=0 of the same build for the five
    permutations and both phases; up to 21 qubits also within 2e-4 of the
    fp64 CPU engine."""
    for inverse in (False, True):
        assert qa.qft_support_plan(width, width, "fp32", 1, inverse)["eligible"]
    _compare(state_runs, width, width, op)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", FALLBACKS, ids=["w%d_l%d" % s for s in FALLBACKS])
def test_fallbacks_unchanged(state_runs, shape, op):
    width, length = shape
    assert not qa.qft_support_plan(length, width, "fp32", 1, op == "iqft")["eligible"]
    _compare(state_runs, width, length, op)


@pytest.fixture(scope="module")
def big_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("support_big")
    mask = (1 << BIG) - 1
    spec = {"width": BIG, "ops": list(OPS), "inputs": [
        [0x5A5A5A5A & mask, _phases()[1]], [mask, _phases()[0]], [1 << (BIG - 1), _phases()[1]]]}
    on = run_child(d / "on.json", ON, "big", spec)
    off = run_child(d / "off.json", OFF, "big", spec)
    return on, off, np.load(str(d / "on.json") + ".npz"), np.load(str(d / "off.json") + ".npz")


@pytest.mark.parametrize("op", OPS)
def test_wide_kernel_reads_through_the_mask(big_runs, op):
    """28 qubits: the sum of the state's raw 32-bit patterns, taken on the
    GPU, and 2^16 seeded sampled amplitudes equal the unrestricted run's."""
    assert [(p["kind"], p["col_lo"], p["n_cols"]) for p in
            qa.qft_support_plan(BIG, BIG, "fp32")["passes"]] == [
        ("mid", 20, 8), ("mid", 12, 8), ("low", 0, 12)]
    on, off, on_s, off_s = big_runs
    for pi in range(3):
        name = "%s_%d" % (op, pi)
        assert abs(on[name]["norm"] - 1.0) < 1e-3, (name, on[name])
        assert on[name]["bitsum"] == off[name]["bitsum"], name
        assert on_s[name].tobytes() == off_s[name].tobytes(), name


@pytest.mark.parametrize("op", OPS)
def test_stale_buffer(op):
    """The benchmark's pattern: a buffer left dense by earlier work, then
    set_permutation and a transform, twice on the same engine. Nothing of the
    old contents may be read."""
    n = 22
    mask = (1 << n) - 1
    p1, p2 = 0x2B3C4D & mask, 0x15A5A5 & mask

    def fresh(p):
        q = qa.create_simulator(n, engine="hip", seed=3)
        q.set_permutation(p, PHASES[1])
        getattr(q, op)(0, n)
        return np.asarray(q.get_state_vector())

    q = qa.create_simulator(n, engine="hip", seed=3)
    for i in range(n):
        q.ry(0.4 + 0.1 * i, i)
    q.set_permutation(p1, PHASES[1])
    getattr(q, op)(0, n)
    first = np.asarray(q.get_state_vector())
    q.set_permutation(p2, PHASES[1])
    getattr(q, op)(0, n)
    second = np.asarray(q.get_state_vector())
    assert first.tobytes() == fresh(p1).tobytes()
    assert second.tobytes() == fresh(p2).tobytes()


@pytest.fixture(scope="module")
def shot_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("support_shots")
    spec = {"widths": [23, 24], "perms": [0x5A5A5A5A, 0x31C5A7]}
    return (
        run_child(d / "on.json", {**ON, "QRACK_GPU_QFT_SUMS": "1"}, "shots", spec),
        run_child(d / "off.json", {**OFF, "QRACK_GPU_QFT_SUMS": "1"}, "shots", spec),
        run_child(d / "nosums.json", {**ON, "QRACK_GPU_QFT_SUMS": "0"}, "shots", spec),
    )


@pytest.mark.parametrize("n", (23, 24))
def test_sampling_after_the_restricted_transform(shot_runs, n):
    on, off, nosums = shot_runs
    for pi in range(2):
        key = "%d_%d" % (n, pi)
        assert sum(c for _, c in on[key]) == 64
        assert on[key] == off[key]
        assert on[key] == nosums[key]


@pytest.mark.parametrize("n", (21, 25))
def test_round_trip_returns_the_basis_state(n):
    p = 0x15A5A5A & ((1 << n) - 1)
    q = qa.create_simulator(n, engine="hip", seed=5)
    q.set_permutation(p)
    q.qft(0, n)
    q.iqft(0, n)
    assert q.multi_shot_measure_mask([1 << i for i in range(n)], 32) == {p: 32}
    q.set_permutation(p)
    q.iqft(0, n)
    q.qft(0, n)
    assert q.multi_shot_measure_mask([1 << i for i in range(n)], 32) == {p: 32}
