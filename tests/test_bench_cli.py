"""bench.py command line: result line, --dump-outputs, --full (CPU engine,
tiny width, so it runs anywhere)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUBITS = 10


def run_bench(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
         "--warmup", "1", "--engine", "cpu", "--qubits", str(QUBITS), *extra],
        capture_output=True, text=True, timeout=120,
    )
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    d1 = tmp_path_factory.mktemp("dump1")
    d2 = tmp_path_factory.mktemp("dump2")
    r1 = run_bench("--dump-outputs", str(d1))
    r2 = run_bench("--dump-outputs", str(d2), "--full")
    return r1, d1, d2, r2


def test_result_line_fields(dumped):
    res = dumped[0]
    assert res["metric"] == "qft_gates_per_sec"
    assert res["unit"] == "gates/s"
    assert res["higher_is_better"] is True
    assert res["dtype"] == "fp32"
    assert res["steps"] == 3
    n_gates = QUBITS + QUBITS * (QUBITS - 1) // 2
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(n_gates * 1000.0 / res["ms_per_step"], rel=1e-9)
    # secondary measurements only run with --full
    assert res["config"]["isolated_h_ms"] is None


def test_dump_is_the_qft_state(dumped):
    d1 = dumped[1]
    names = sorted(os.listdir(d1))
    assert names == ["sample_counts.npy", "sample_keys.npy", "state_amps.npy", "state_index.npy"]
    arrays = {n: np.load(os.path.join(d1, n)) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2**20

    assert arrays["sample_counts.npy"].sum() == 1
    assert 0 <= arrays["sample_keys.npy"][0] < 2**QUBITS

    # a state this small is dumped whole: the QFT of a basis state has
    # uniform modulus and unit norm
    idx = arrays["state_index.npy"]
    amps = arrays["state_amps.npy"]
    assert np.array_equal(idx, np.arange(2**QUBITS))
    assert amps.shape == (2**QUBITS, 2) and amps.dtype == np.float32
    mod2 = (amps.astype(np.float64) ** 2).sum(axis=1)
    assert np.allclose(mod2, 2.0**-QUBITS, rtol=1e-4)


def test_dump_repeats_and_full_leaves_it_alone(dumped):
    d1, d2 = dumped[1:3]
    for n in os.listdir(d1):
        assert np.array_equal(np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))), n


def test_full_adds_isolated_gate_timing(dumped):
    assert dumped[3]["config"]["isolated_h_ms"] > 0


def test_large_state_is_sampled_at_fixed_places(tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)

    class Stub:
        def get_amplitude_page(self, offset, length):
            i = np.arange(offset, offset + length)
            return (i + 1j * (i % 7)).astype(np.complex128)

    n_amps = 1 << 26
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), Stub(), n_amps, {5: 1}, "fp64")
    idx = np.load(tmp_path / "a" / "state_index.npy")
    amps = np.load(tmp_path / "a" / "state_amps.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "state_index.npy"))
    assert len(idx) == bench.DUMP_CHUNKS * bench.DUMP_CHUNK_LEN
    assert amps.dtype == np.float64 and amps.shape == (len(idx), 2)
    assert idx[0] == 0 and idx[-1] == n_amps - 1
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(amps[:, 0], idx) and np.array_equal(amps[:, 1], idx % 7)
    assert idx.nbytes + amps.nbytes <= 64 * 2**20
