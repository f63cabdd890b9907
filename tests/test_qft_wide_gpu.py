"""Wide-tile QFT mid pass (8 or 9 columns per state pass) of the HIP engine.

QRACK_GPU_QFT_MIDMAX, _LAZYPERM and _SUMS are read once per process, so each
setting runs in its own child process. A child does the heavy part where
the state is: at n = 20 and 21 it compares every state with the fp64 CPU
engine itself (assert_states_close, largest |d amp|, a digest of the bytes)
and reports numbers; at n >= 22 it reports the state's norm and the
amplitudes at 2^16 seeded indices, gathered on the GPU, and the default
schedule's samples are held against those of QRACK_GPU_QFT_MIDMAX=6, the
schedule the rest of the suite vouches for. A uniform sample of that size
meets every one of the 2^13 positions of a wide tile eight times on
average and every tile-sized stretch of the state at n = 27 four times.
"""
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
TESTS = os.path.dirname(os.path.abspath(__file__))
PHASES = ((1.0, 0.0), (float(np.cos(0.7)), float(np.sin(0.7))))
TOL = 2e-4  # the fp32 tolerance of the existing QFT GPU tests
EPS32 = float(np.finfo(np.float32).eps)

# (engine width, register length); the wide pass each one must select
SHAPES = {
    (20, 20): ("mid", 12, 8),
    (21, 21): ("mid", 12, 9),
    (22, 21): ("mid", 12, 9),
    (23, 23): ("mid", 14, 9),
    (25, 25): ("mid", 16, 9),
    (27, 27): ("mid", 18, 9),
    (23, 21): ("mid", 12, 9),
}
# 22 full-width ties at three passes (6 + 4 + 12 against 9 + 9 + 4) and a tie
# keeps the 64-wide kernel, so it carries no wide pass; it is run all the
# same, and the 21-qubit register of a 22-qubit engine stands in above.
TIED_SHAPE = (22, 22)
ALL_SHAPES = tuple(SHAPES) + (TIED_SHAPE,)
OPS = ("qft", "iqft")
CPU_SHAPES = ((20, 20), (21, 21))

# largest |d amp| against the fp64 CPU engine: the default schedule may
# exceed the MIDMAX=6 schedule's by this factor at most. Within a K-column
# group the ramps of the lower columns are f0^(2^m), m < K, taken by
# repeated squaring of the one sincos f0, so the rounding of f0's angle
# reaches a column multiplied by up to 2^(K-1). The 8-column pass is two
# K=4 groups where the old schedule has K=3 and K=2 groups: at worst twice
# the old schedule's ramp error, nothing else differs. The 9-column pass is
# three K=3 groups like the 6- and 3-column passes it replaces. Measured
# (profiles/PROF_QFT_WIDE_MID.md): 0.97 to 1.66 at n = 20, exactly 1 at
# n = 21, where the states are bit-identical.
DAMP_FACTOR = 2.0


def perms_for(width):
    mask = (1 << width) - 1
    return (0, mask, 0x5A5A5A5A & mask, 1 << (width - 1), 1)


def inputs_for(width):
    """(key, kind, perm, phase): lazy basis states, the same after one x
    gate (materialised), and the skewed state."""
    out = []
    for pi, perm in enumerate(perms_for(width)):
        for fi, ph in enumerate(PHASES):
            out.append(("lazy_%d_%d" % (pi, fi), "lazy", perm, ph))
            out.append(("x_%d_%d" % (pi, fi), "x", perm, ph))
    out.append(("skew", "skew", 5, (1.0, 0.0)))
    return out


_CHILD = r"""
import hashlib, json, sys
import torch
torch.cuda.init()  # torch first, engine second
root, tests, out, mode = sys.argv[1:5]
spec = json.loads(sys.argv[5])
sys.path.insert(0, root)
sys.path.insert(0, tests)
import numpy as np
import qrack_amd as qa
from ref_sim import assert_states_close

def prepare(q, width, kind, perm, ph):
    if kind == "skew":
        q.set_permutation(5)
        for i in range(0, width, 4):
            q.ry(0.9 + 0.05 * i, i)
    else:
        q.set_permutation(perm, complex(*ph))
        if kind == "x":
            q.x(0)

def view(q, width):
    q.finish()
    return torch.from_dlpack(q.dlpack_view(0, 1 << width))

res = {}
samples = {}
if mode == "states":
    for width, length, op, with_cpu, inputs in spec["cases"]:
        idx = None
        if not with_cpu:
            g = torch.Generator().manual_seed(20240229 + width)
            idx = torch.randint(0, 1 << width, (1 << 16,), generator=g).cuda()
        for key, kind, perm, ph in inputs:
            q = qa.create_simulator(width, engine="hip", seed=1)
            prepare(q, width, kind, perm, ph)
            getattr(q, op)(0, length)
            name = "%d_%d_%s_%s" % (width, length, op, key)
            if with_cpu:
                got = np.asarray(q.get_state_vector())
                cp = qa.create_simulator(width, engine="cpu", precision="fp64", seed=1)
                prepare(cp, width, kind, perm, ph)
                getattr(cp, op)(0, length)
                want = np.asarray(cp.get_state_vector())
                err = None
                try:
                    assert_states_close(got, want, spec["tol"])
                except AssertionError as e:
                    err = str(e)
                res[name] = {
                    "close_err": err,
                    "damp": float(np.max(np.abs(got.astype(np.complex128) - want))),
                    "sha": hashlib.sha256(got.tobytes()).hexdigest(),
                }
            else:
                t = view(q, width)
                samples[name] = t[idx].cpu().numpy()
                res[name] = {
                    "norm": float(torch.linalg.vector_norm(torch.view_as_real(t).double()).item()),
                }
            del q
    np.savez(out + ".npz", **samples)
elif mode == "hashes":
    for width, length, op, inputs in spec["cases"]:
        for key, kind, perm, ph in inputs:
            q = qa.create_simulator(width, engine="hip", seed=1)
            prepare(q, width, kind, perm, ph)
            getattr(q, op)(0, length)
            got = np.asarray(q.get_state_vector())
            res["%d_%d_%s_%s" % (width, length, op, key)] = hashlib.sha256(got.tobytes()).hexdigest()
elif mode == "roundtrip":
    for width in spec["widths"]:
        q = qa.create_simulator(width, engine="hip", seed=1)
        prepare(q, width, "skew", 5, (1.0, 0.0))
        before = view(q, width).clone()
        torch.cuda.synchronize()  # the copy runs on torch's stream, the transform on the engine's
        q.qft(0, width)
        q.iqft(0, width)
        after = view(q, width)
        inner = torch.sum(torch.conj(before).to(torch.complex128) * after.to(torch.complex128))
        res[str(width)] = {
            "fid": float(torch.abs(inner).item()),
            "dmax": float(torch.max(torch.abs(after - before)).item()),
            "amax": float(torch.max(torch.abs(before)).item()),
        }
elif mode == "shots":
    for n in spec["widths"]:
        pows = [1 << i for i in range(n)]
        q = qa.create_simulator(n, engine="hip", seed=7)
        q.set_permutation(0x5A5A5A5A & ((1 << n) - 1))
        q.qft(0, n)
        uni = q.multi_shot_measure_mask(pows, 64)
        q.set_permutation(5)
        for i in range(0, n, 4):
            q.ry(0.9 + 0.05 * i, i)
        q.qft(0, n)
        skew = q.multi_shot_measure_mask(pows, 64)
        res[str(n)] = [sorted(uni.items()), sorted(skew.items())]
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


def _state_cases():
    return [[w, l, op, (w, l) in CPU_SHAPES, inputs_for(w)]
            for (w, l) in ALL_SHAPES for op in OPS]


@pytest.fixture(scope="module")
def state_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_states")
    spec = {"cases": _state_cases(), "tol": TOL}
    wide = run_child(d / "wide.json", {"QRACK_GPU_QFT_MIDMAX": "9"}, "states", spec)
    six = run_child(d / "six.json", {"QRACK_GPU_QFT_MIDMAX": "6"}, "states", spec)
    return wide, six, np.load(str(d / "wide.json") + ".npz"), np.load(str(d / "six.json") + ".npz")


@pytest.mark.parametrize("shape", list(SHAPES), ids=["w%d_l%d" % s for s in SHAPES])
def test_shape_selects_a_wide_pass(shape):
    width, length = shape
    plan = [tuple(p) for p in qa.qft_pass_plan(length, width, "fp32")]
    assert SHAPES[shape] in plan, plan
    assert all(nc <= 6 for kind, lo, nc in qa.qft_pass_plan(length, width, "fp32", 6)
               if kind == "mid")


def test_tied_shape_keeps_the_64_wide_kernel():
    width, length = TIED_SHAPE
    assert [tuple(p) for p in qa.qft_pass_plan(length, width, "fp32")] == [
        ("mid", 16, 6), ("mid", 12, 4), ("low", 0, 12)]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=["n%d" % s[0] for s in CPU_SHAPES])
def test_against_fp64_cpu_engine(state_runs, shape, op):
    """assert_states_close at 2e-4 for every input, and the largest |d amp|
    no more than DAMP_FACTOR times the MIDMAX=6 schedule's on that input."""
    wide, six = state_runs[:2]
    width, length = shape
    for key, _, _, _ in inputs_for(width):
        name = "%d_%d_%s_%s" % (width, length, op, key)
        w, s = wide[name], six[name]
        print(name, "damp wide %.4e six %.4e ratio %.3f" % (
            w["damp"], s["damp"], w["damp"] / s["damp"] if s["damp"] else float("inf")))
        assert w["close_err"] is None, (name, w["close_err"])
        assert s["close_err"] is None, (name, s["close_err"])
        assert w["damp"] <= DAMP_FACTOR * s["damp"], (name, w["damp"], s["damp"])


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize(
    "shape", [s for s in ALL_SHAPES if s not in CPU_SHAPES],
    ids=["w%d_l%d" % s for s in ALL_SHAPES if s not in CPU_SHAPES])
def test_against_six_column_schedule(state_runs, shape, op):
    wide, six, wide_samples, six_samples = state_runs
    width, length = shape
    for key, _, _, _ in inputs_for(width):
        name = "%d_%d_%s_%s" % (width, length, op, key)
        w, s = wide[name], six[name]
        assert abs(w["norm"] - 1.0) < 1e-3 and abs(s["norm"] - 1.0) < 1e-3, (name, w["norm"])
        got = wide_samples[name].astype(np.complex128)
        ref = six_samples[name].astype(np.complex128)
        scale = np.linalg.norm(ref)
        assert scale > 0
        assert_states_close(got / scale, ref / scale, TOL)
        # amplitude by amplitude as well. Each of the `length` columns is a
        # butterfly and a phase whose angle, sincos and products carry a few
        # ulps; 8 ulps a column, added up linearly over either schedule, is
        # the most two fp32 runs of the same transform can differ by.
        dmax = float(np.max(np.abs(got - ref)))
        assert dmax <= 8 * length * EPS32 * float(np.max(np.abs(ref))), (name, dmax)


@pytest.fixture(scope="module")
def eager_hashes(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_eager")
    cases = [[w, l, op, [i for i in inputs_for(w) if i[1] == "lazy"]]
             for (w, l) in CPU_SHAPES for op in OPS]
    return run_child(d / "eager.json",
                     {"QRACK_GPU_QFT_MIDMAX": "9", "QRACK_GPU_QFT_LAZYPERM": "0"},
                     "hashes", {"cases": cases})


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=["n%d" % s[0] for s in CPU_SHAPES])
def test_lazy_first_pass_bit_equal_to_eager(state_runs, eager_hashes, shape, op):
    wide = state_runs[0]
    width, length = shape
    for key, kind, _, _ in inputs_for(width):
        if kind != "lazy":
            continue
        name = "%d_%d_%s_%s" % (width, length, op, key)
        assert wide[name]["sha"] == eager_hashes[name], f"{name}: not bit-equal to the eager run"


@pytest.fixture(scope="module")
def roundtrips(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_roundtrip")
    return run_child(d / "rt.json", {"QRACK_GPU_QFT_MIDMAX": "9"}, "roundtrip",
                     {"widths": [21, 25]})


@pytest.mark.parametrize("width", (21, 25))
def test_qft_then_iqft_returns_the_input(roundtrips, width):
    r = roundtrips[str(width)]
    assert r["fid"] > 1.0 - TOL, r
    # two transforms, 8 ulps a column each (see above), on the largest amplitude
    assert r["dmax"] <= 2 * 8 * width * EPS32 * r["amax"], r


@pytest.fixture(scope="module")
def shot_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_shots")
    spec = {"widths": [23, 24]}
    on = run_child(d / "on.json", {"QRACK_GPU_QFT_MIDMAX": "9", "QRACK_GPU_QFT_SUMS": "1"},
                   "shots", spec)
    off = run_child(d / "off.json", {"QRACK_GPU_QFT_MIDMAX": "9", "QRACK_GPU_QFT_SUMS": "0"},
                    "shots", spec)
    return on, off


@pytest.mark.parametrize("n", (23, 24))
def test_sampling_from_tile_sums_after_the_wide_schedule(shot_runs, n):
    on, off = shot_runs
    assert on[str(n)] == off[str(n)]
    assert sum(c for _, c in on[str(n)][0]) == 64 and sum(c for _, c in on[str(n)][1]) == 64
