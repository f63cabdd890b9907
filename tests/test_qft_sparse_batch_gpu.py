"""Last low pass of a QFT of a basis state, tiles taken in batches.

k_qft_low_sparse_last runs the groups at gLo = 8 and gLo = 4 for a batch of
four tiles at once on compact images, then the group at gLo = 0 and the
write-out tile by tile with each wave on its own quarter, and leaves the
tile sums after the batch. With QRACK_GPU_QFT_SPARSELAST=0 the dense kernel
runs every orbit of every tile. Every stored value goes through the same
instructions either way, so the states must be equal byte for byte, and the
tile sums equal as doubles. The switch is read once per process, so each
setting runs in its own child process; all widths of one grid setting share
one pair of children.
"""
import cmath
import json
import os
import subprocess
import sys

import pytest

import qrack_amd as qa

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# width -> (columns of the last pass, tiles it runs), by hand from qft_plan.hpp:
# 14 is the narrowest eligible width and one batch, 15 two batches, 17 the
# smallest 8-column ladder
PLAN = {14: (12, 4), 15: (12, 8), 17: (8, 32), 20: (12, 256)}
SUMS_PLAN = {23: (8, 2048), 24: (12, 4096)}  # maxQPower >= 2^23: tile sums are left
# 1 and i make signed zeros in the butterflies; the last is a generic global phase
PHASES = (1 + 0j, 1j, cmath.exp(0.7j))
ON = {"QRACK_GPU_QFT_SPARSELAST": "1"}
OFF = {"QRACK_GPU_QFT_SPARSELAST": "0"}
# the default grid (a block per batch), one block walking every batch, and
# three blocks striding over them (8 batches of width 17: 3, 3, 2)
GRIDS = {"default": (), "one_block": (("QRACK_GPU_BLOCKS", "1"),),
         "three_blocks": (("QRACK_GPU_BLOCKS", "3"),)}


def perms_for(width):
    """All zeros, all ones, the benchmark's pattern, and one whose low 12
    bits (0xA53) make slot and below nonzero in every group."""
    mask = (1 << width) - 1
    return (0, mask, 0x5A5A5A5A & mask, ((0x2B5000 & ~0xFFF) | 0xA53) & mask)


def restore_perms(width):
    """Back to back on one engine: same width, different low 12 bits, then the
    first again, so each meets the template the other left."""
    mask = (1 << width) - 1
    a, b = 0x2B3A53 & mask, 0x2B35AC & mask
    return (a, b, a)


_CHILD = r"""
import hashlib, json, sys
root, out = sys.argv[1:3]
spec = json.loads(sys.argv[3])
sys.path.insert(0, root)
import numpy as np
import qrack_amd as qa

res = {}
for name, width, op, perms, phases, shots in spec["cases"]:
    q = qa.create_simulator(width, engine="hip", seed=11)
    for pi, perm in enumerate(perms):
        for fi, (re, im) in enumerate(phases):
            q.set_permutation(perm, complex(re, im))
            getattr(q, op)(0, width)
            entry = {}
            if shots:
                # first, while the tile sums of the pass are what is left
                pows = [1 << i for i in range(width)]
                entry["shots"] = sorted(q.multi_shot_measure_mask(pows, shots).items())
            got = np.ascontiguousarray(q.get_state_vector())
            entry["sha"] = hashlib.sha256(got.data).hexdigest()
            res["%s_%d_%d" % (name, pi, fi)] = entry
    del q
json.dump(res, open(out, "w"))
print("CHILD_OK")
"""


def run_child(out, env_extra, spec):
    env = {**os.environ, **env_extra}
    r = subprocess.run(
        [sys.executable, "-c", _CHILD, ROOT, str(out), json.dumps(spec)],
        env=env, capture_output=True, text=True, timeout=600,
    )
    assert "CHILD_OK" in r.stdout, f"stdout={r.stdout[-2000:]}\nstderr={r.stderr[-4000:]}"
    return json.load(open(out))


def _phases():
    return [[ph.real, ph.imag] for ph in PHASES]


def _grid_spec():
    cases = []
    for width in sorted(PLAN):
        cases.append(["qft%d" % width, width, "qft", list(perms_for(width)), _phases(), 0])
        cases.append(["restore%d" % width, width, "qft", list(restore_perms(width)),
                      _phases()[2:], 0])
    cases.append(["iqft17", 17, "iqft", list(perms_for(17)), _phases()[2:], 0])
    return {"cases": cases}


class _Runs:
    """Switch-on and switch-off children of one grid setting, started when
    first asked for."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.cache = {}

    def get(self, grid):
        if grid not in self.cache:
            env = dict(GRIDS[grid])
            self.cache[grid] = (
                run_child(self.tmp / ("on_%s.json" % grid), {**env, **ON}, _grid_spec()),
                run_child(self.tmp / ("off_%s.json" % grid), {**env, **OFF}, _grid_spec()),
            )
        return self.cache[grid]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return _Runs(tmp_path_factory.mktemp("sparse_batch"))


def _assert_plan(width, n_cols, tiles):
    """The plan must end in the low ladder the case is about: a planner
    change then fails here and does not silently skip the kernel."""
    plan = qa.qft_support_plan(width, width, "fp32", 1)
    assert plan["eligible"]
    last = plan["passes"][-1]
    assert (last["kind"], last["n_cols"], last["active_tiles"]) == ("low", n_cols, tiles)
    assert qa.qft_sparse_last_plan(n_cols, 0xA53)["eligible"]


def _compare(on, off, name, n_perms, n_phases):
    for pi in range(n_perms):
        for fi in range(n_phases):
            key = "%s_%d_%d" % (name, pi, fi)
            assert on[key]["sha"] == off[key]["sha"], f"{key}: differs from the dense last pass"


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("width", sorted(PLAN))
def test_bit_equal_to_the_dense_last_pass(runs, width, grid):
    """SHA-256 of the whole state, four permutations by three phases, on the
    default grid and with one and three blocks walking the batches."""
    _assert_plan(width, *PLAN[width])
    on, off = runs.get(grid)
    _compare(on, off, "qft%d" % width, 4, len(PHASES))


@pytest.mark.parametrize("grid", ("default", "one_block"))
@pytest.mark.parametrize("width", sorted(PLAN))
def test_template_is_restored(runs, width, grid):
    """Two permutations with different low 12 bits back to back on one
    engine, and the first again: each block must have given the LDS template
    back, and the engine its device template."""
    _assert_plan(width, *PLAN[width])
    on, off = runs.get(grid)
    _compare(on, off, "restore%d" % width, 3, 1)
    assert on["restore%d_0_0" % width]["sha"] == on["restore%d_2_0" % width]["sha"]
    assert on["restore%d_0_0" % width]["sha"] != on["restore%d_1_0" % width]["sha"]


def test_inverse_unchanged(runs):
    """iqft takes the dense support kernel; the switch must not move it."""
    on, off = runs.get("default")
    _compare(on, off, "iqft17", 4, 1)


@pytest.fixture(scope="module")
def sums_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sparse_batch_sums")
    cases = [["sums%d" % w, w, "qft", [0x5A5A5A5A & ((1 << w) - 1), 0x31CA53], _phases()[2:], 64]
             for w in sorted(SUMS_PLAN)]
    spec = {"cases": cases}
    env = {"QRACK_GPU_QFT_SUMS": "1"}
    return (run_child(d / "on.json", {**env, **ON}, spec),
            run_child(d / "off.json", {**env, **OFF}, spec))


@pytest.mark.parametrize("width", sorted(SUMS_PLAN))
def test_tile_sums_and_state(sums_runs, width):
    """Where the pass leaves the tile sums: the state, and 64 seeded shots
    drawn through those sums, against the dense kernel's."""
    _assert_plan(width, *SUMS_PLAN[width])
    on, off = sums_runs
    for pi in range(2):
        key = "sums%d_%d_0" % (width, pi)
        assert sum(c for _, c in on[key]["shots"]) == 64
        assert on[key]["shots"] == off[key]["shots"]
        assert on[key]["sha"] == off[key]["sha"]
