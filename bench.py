#!/usr/bin/env python3
"""qrack_amd flagship benchmark — QFT wall-clock on the HIP state-vector
engine, the reference's headline protocol (the test_qft_* cases of its
benchmark suite).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
launched via torch.distributed.run with one rank per GPU over RCCL. One step
= state re-init + full n-qubit QFT + 1-shot terminal sample. Weak scaling:
qubits = base_qubits + log2(N), so per-GPU amplitude count is fixed.

Rank 0 prints ONE JSON line with the whole-job aggregate `qft_gates_per_sec`
(gates applied per second across the whole job; ms_per_step = one full QFT).

A plain run does only that: set up, warm up, time the K steps, print the line.
`--dump-outputs DIR` additionally writes what the last timed step computed
(its terminal sample and a fixed, seeded sample of the final state) as
DIR/<name>.npy, so two builds can be compared output for output.
`--full` adds the secondary measurements (isolated single-gate H wall-clock).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# --dump-outputs state sample: DUMP_CHUNKS contiguous runs of DUMP_CHUNK_LEN
# amplitudes at seeded offsets (first and last run always included); states
# no larger than the sample are written whole. 2^19 amplitudes -> 4 MB of
# fp32 (8 MB of fp64) re/im pairs plus 4 MB of indices.
DUMP_CHUNKS = 32
DUMP_CHUNK_LEN = 1 << 14
DUMP_SEED = 20240229


def dump_outputs(out_dir, engine_sim, n_amps, sample, precision):
    """Write the last timed step's outputs as <name>.npy under out_dir.

    sample_keys/sample_counts: the terminal multi-shot sample the step returned.
    state_index/state_amps: amplitudes (re, im columns) of the state the step
    left behind, at the fixed indices in state_index.
    """
    os.makedirs(out_dir, exist_ok=True)
    real = np.float32 if precision == "fp32" else np.float64

    keys = sorted(sample)
    np.save(os.path.join(out_dir, "sample_keys.npy"), np.asarray(keys, dtype=np.float64))
    np.save(os.path.join(out_dir, "sample_counts.npy"),
            np.asarray([sample[k] for k in keys], dtype=np.float64))

    if n_amps <= DUMP_CHUNKS * DUMP_CHUNK_LEN:
        runs = [(0, n_amps)]
    else:
        n_runs = n_amps // DUMP_CHUNK_LEN
        rng = np.random.default_rng(DUMP_SEED)
        picks = rng.choice(n_runs - 2, size=DUMP_CHUNKS - 2, replace=False) + 1
        starts = sorted({0, n_runs - 1, *(int(x) for x in picks)})
        runs = [(s * DUMP_CHUNK_LEN, DUMP_CHUNK_LEN) for s in starts]

    index = np.concatenate([np.arange(o, o + n, dtype=np.float64) for o, n in runs])
    amps = np.concatenate([np.asarray(engine_sim.get_amplitude_page(o, n)) for o, n in runs])
    pairs = np.stack([amps.real, amps.imag], axis=1).astype(real)
    np.save(os.path.join(out_dir, "state_index.npy"), index)
    np.save(os.path.join(out_dir, "state_amps.npy"), pairs)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--qubits", type=int, default=0, help="base (per-GPU) qubit count; 0 = auto")
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp64"])
    p.add_argument("--engine", default="auto", choices=["auto", "hip", "cpu"])
    p.add_argument("--backend", default="auto",
                   help="torch.distributed backend override (auto = cpu:gloo,cuda:nccl for hip)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (isolated single-gate H)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = max(args.gpus, world)

    if world > 1:
        # ORDER MATTERS: torch.cuda must initialize the HIP runtime BEFORE
        # the qrack_amd extension touches it — the reverse order leaves
        # torch.cuda reporting "No HIP GPUs are available" in this process
        import torch

        if torch.cuda.is_available():
            torch.cuda.init()

    import qrack_amd as qa

    engine = args.engine
    if engine == "auto":
        engine = "hip" if qa.hip_device_count() > 0 else "cpu"

    # base width: 30 qubits fp32 on GPU (8.6 GB state; QFT ~= 494 gates);
    # tiny on CPU so the no-GPU smoke path finishes instantly
    base_qubits = args.qubits or (30 if engine == "hip" else 16)

    dist = None
    if world > 1:
        import torch
        import torch.distributed as tdist

        # mixed backend: CUDA tensors (half-page exchanges) over RCCL/xGMI,
        # CPU tensors (norm scalars, decision broadcasts, object gathers)
        # over gloo — a pure nccl group rejects CPU-tensor collectives
        backend = args.backend
        if backend == "auto":
            backend = "cpu:gloo,cuda:nccl" if engine == "hip" else "gloo"
        tdist.init_process_group(backend=backend)
        if engine == "hip":
            # clamp for single-GPU multi-rank rehearsals; identity on real
            # one-rank-per-GPU launches
            local_rank = local_rank % max(1, qa.hip_device_count())
            torch.cuda.set_device(local_rank)
        dist = tdist

    meta_bits = (world - 1).bit_length() if world > 1 else 0
    qubits = base_qubits + meta_bits

    if world > 1:
        from qrack_amd.dist_pager import DistQPager

        sim = DistQPager(qubits, precision=args.precision, engine=engine, seed=42,
                         device_id=local_rank)
    else:
        sim = qa.create_simulator(
            qubits, precision=args.precision, engine=engine, seed=42, device_id=local_rank
        )

    n_gates = qubits + qubits * (qubits - 1) // 2  # H + controlled-phase count

    def step():
        sim.set_permutation(0x5A5A5A5A & ((1 << qubits) - 1))
        sim.qft(0, qubits)
        return sim.multi_shot_measure_mask([1 << i for i in range(min(qubits, 16))], 1)

    def sync():
        if dist is not None:
            dist.barrier()
        if engine == "hip" and world > 1:
            import torch

            torch.cuda.synchronize()
        if hasattr(sim, "finish"):
            sim.finish()

    for _ in range(args.warmup):
        step()
    sync()

    t0 = time.perf_counter()
    for _ in range(args.steps):
        last_sample = step()
    sync()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    # MAX over ranks
    if dist is not None:
        import torch

        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = 1000.0 * elapsed / args.steps
    gates_per_sec = n_gates * args.steps / elapsed
    single_gate_ms = ms_per_step / n_gates

    # what the timed path left behind: its last sample and the final state
    # (on a multi-rank job, rank 0's sample and its local page)
    if args.dump_outputs and rank == 0:
        local = sim.q if world > 1 else sim
        dump_outputs(args.dump_outputs, local, 1 << (qubits - meta_bits),
                     dict(last_sample), args.precision)

    # Isolated single-gate wall-clock (the BASELINE.md metric): one H on a
    # low qubit, synchronized each application — not amortized across fused
    # QFT columns. Measured with --full, on the single-rank path only.
    isolated_h_ms = None
    if args.full and world == 1:
        sim.set_permutation(0)
        reps = 10
        sim.h(0)
        if hasattr(sim, "finish"):
            sim.finish()
        th0 = time.perf_counter()
        for _ in range(reps):
            sim.h(0)
            if hasattr(sim, "finish"):
                sim.finish()
        th1 = time.perf_counter()
        isolated_h_ms = 1000.0 * (th1 - th0) / reps

    if rank == 0:
        out = {
            "metric": "qft_gates_per_sec",
            "value": gates_per_sec,
            "unit": "gates/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.precision,
            "data": "synthetic",
            "config": {
                "model": "qft",
                "qubits": qubits,
                "base_qubits_per_gpu": base_qubits,
                "n_gates": n_gates,
                "single_gate_ms": single_gate_ms,
                "isolated_h_ms": isolated_h_ms,
                # capacity headline (measured: profiles/qft_fuse4.csv runs
                # the 34-qubit = 128 GB fp32 QFT at fidelity 1.0)
                "max_full_state_qubits_fp32": 34,
                "engine": engine,
                "global_batch": 1,
                "seq_len": qubits,
                "parallelism": f"pager{world}" if world > 1 else "single",
            },
        }
        print(json.dumps(out))

    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
