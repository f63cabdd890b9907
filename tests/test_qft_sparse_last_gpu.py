"""Last low pass of a QFT of a lazy basis state, orbits with a nonzero only.

With QRACK_GPU_QFT_SPARSELAST on (the default) the forward last pass of a
support-restricted transform (8 or 12 columns) runs the one, sixteen and 256
orbits per tile that hold a nonzero input and takes their zero partners from
a template of signed zeros; with =0 it runs every orbit of every tile
(qa.qft_sparse_last_plan gives the schedule). Every stored value goes
through the same instructions either way, signed zeros included, so the
states must be equal byte for byte. The switch is read once per process, so
each setting runs in its own child process.
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
# 1, -1, i, -i make signed zeros in the butterflies; the last is generic
PHASES = (1 + 0j, -1 + 0j, 1j, -1j, cmath.exp(0.7j))
# width -> columns of the last pass: 14 is 4 tiles, 15 is 8 tiles,
# 17 and 23 have the 8-column ladder, 22 and 23 two mid passes ahead
WIDTHS = {14: 12, 15: 12, 17: 8, 18: 12, 20: 12, 22: 12, 23: 8}
CAPPED = (18, 17)  # again with a grid of 3 blocks striding over the tiles
ON = {"QRACK_GPU_QFT_SPARSELAST": "1"}
OFF = {"QRACK_GPU_QFT_SPARSELAST": "0"}


def perms_for(width):
    """The five of the support test, and four whose low 12 bits put the
    nonzero orbit and its slot in every position class."""
    mask = (1 << width) - 1
    base = (0, mask, 0x5A5A5A5A & mask, 1 << (width - 1), 1)
    top = 0x2B5000 & mask & ~0xFFF
    return base + tuple(top | low for low in (0x00F, 0x0F0, 0xF00, 0xA5A))


_CHILD = r"""
import hashlib, json, sys
root, out, mode = sys.argv[1:4]
spec = json.loads(sys.argv[4])
sys.path.insert(0, root)
import numpy as np
import qrack_amd as qa

res = {}
if mode == "states":
    for width, op, perms, phases in spec["cases"]:
        q = qa.create_simulator(width, engine="hip", seed=1)
        for pi, perm in enumerate(perms):
            for fi, (re, im) in enumerate(phases):
                q.set_permutation(perm, complex(re, im))
                getattr(q, op)(0, width)
                got = np.ascontiguousarray(q.get_state_vector())
                # the norm does not depend on the phase: once per permutation,
                # summed in fp64 (an fp32 sum over 2^23 terms is off by 1e-3)
                norm = None
                if fi == len(phases) - 1:
                    norm = float(np.square(got.view(got.real.dtype), dtype=np.float64).sum())
                res["%d_%s_%d_%d" % (width, op, pi, fi)] = {
                    "sha": hashlib.sha256(got.data).hexdigest(),
                    "norm": norm,
                }
        del q
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
        [sys.executable, "-c", _CHILD, ROOT, str(out), mode, json.dumps(spec)],
        env=env, capture_output=True, text=True, timeout=600,
    )
    assert "CHILD_OK" in r.stdout, f"stdout={r.stdout[-2000:]}\nstderr={r.stderr[-4000:]}"
    return json.load(open(out))


def _phases():
    return [[ph.real, ph.imag] for ph in PHASES]


class _StateRuns:
    """Switch-on and switch-off children of one (width, op, extra environment),
    started when first asked for."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.cache = {}

    def get(self, width, op, extra=()):
        key = (width, op, extra)
        if key not in self.cache:
            tag = "%d_%s_%d" % (width, op, len(self.cache))
            spec = {"cases": [[width, op, list(perms_for(width)), _phases()]]}
            env = dict(extra)
            self.cache[key] = (
                run_child(self.tmp / ("on_%s.json" % tag), {**env, **ON}, "states", spec),
                run_child(self.tmp / ("off_%s.json" % tag), {**env, **OFF}, "states", spec),
            )
        return self.cache[key]


@pytest.fixture(scope="module")
def state_runs(tmp_path_factory):
    return _StateRuns(tmp_path_factory.mktemp("sparse_last_states"))


def _compare(state_runs, width, op, extra=()):
    on, off = state_runs.get(width, op, extra)
    for pi in range(len(perms_for(width))):
        for fi in range(len(PHASES)):
            name = "%d_%s_%d_%d" % (width, op, pi, fi)
            if on[name]["norm"] is not None:
                assert abs(on[name]["norm"] - 1.0) < 1e-3, (name, on[name])
            assert on[name]["sha"] == off[name]["sha"], f"{name}: differs from the switch-off run"


def _last_pass(width):
    plan = qa.qft_support_plan(width, width, "fp32", 1)
    assert plan["eligible"]
    return plan["passes"][-1]


@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_bit_equal_to_the_dense_last_pass(state_runs, width):
    """SHA-256 of the whole state, nine permutations by five phases."""
    last = _last_pass(width)
    assert (last["kind"], last["n_cols"]) == ("low", WIDTHS[width])
    assert qa.qft_sparse_last_plan(last["n_cols"], 1)["eligible"]
    _compare(state_runs, width, "qft")


@pytest.mark.parametrize("width", CAPPED)
def test_bit_equal_under_a_capped_grid(state_runs, width):
    """QRACK_GPU_BLOCKS=3: 64 and 32 tiles strided over 3 blocks, so a block
    takes the template back from its own write-out tile after tile."""
    assert _last_pass(width)["active_tiles"] in (64, 32)
    _compare(state_runs, width, "qft", (("QRACK_GPU_BLOCKS", "3"),))


@pytest.mark.parametrize("width,op", ((16, "iqft"), (19, "qft")))
def test_other_paths_unchanged(state_runs, width, op):
    """The inverse transform and a plan with a register-column pass do not
    take the new kernel; the switch must not move them."""
    if op == "qft":
        assert not qa.qft_support_plan(width, width, "fp32", 1)["eligible"]
    _compare(state_runs, width, op)


@pytest.fixture(scope="module")
def shot_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sparse_last_shots")
    spec = {"widths": [23, 24], "perms": [0x5A5A5A5A, 0x31C5A7]}
    return (
        run_child(d / "on.json", {**ON, "QRACK_GPU_QFT_SUMS": "1"}, "shots", spec),
        run_child(d / "off.json", {**OFF, "QRACK_GPU_QFT_SUMS": "1"}, "shots", spec),
    )


@pytest.mark.parametrize("n", (23, 24))
def test_sampling_uses_the_same_tile_sums(shot_runs, n):
    """64 seeded shots through the per-tile norms the last pass leaves."""
    on, off = shot_runs
    for pi in range(2):
        key = "%d_%d" % (n, pi)
        assert sum(c for _, c in on[key]) == 64
        assert on[key] == off[key]


@pytest.mark.parametrize("n", (17, 20))
def test_stale_buffer(n):
    """A buffer left dense by earlier work, then set_permutation and qft,
    twice on the same engine: nothing outside the support may be read."""
    mask = (1 << n) - 1
    p1, p2 = 0x2B3C4D & mask, 0x15A5A5 & mask
    phase = PHASES[2]

    def fresh(p):
        q = qa.create_simulator(n, engine="hip", seed=3)
        q.set_permutation(p, phase)
        q.qft(0, n)
        return np.asarray(q.get_state_vector())

    q = qa.create_simulator(n, engine="hip", seed=3)
    for i in range(n):
        q.ry(0.4 + 0.1 * i, i)
    q.set_permutation(p1, phase)
    q.qft(0, n)
    first = np.asarray(q.get_state_vector())
    q.set_permutation(p2, phase)
    q.qft(0, n)
    second = np.asarray(q.get_state_vector())
    assert first.tobytes() == fresh(p1).tobytes()
    assert second.tobytes() == fresh(p2).tobytes()
