"""pauli_rotation and evolve_pauli_sum on the HIP engine: one in-place
read-and-write pass per planned pass.

Oracle and bounds: pauli_evolve_oracle (numpy float64, per-term factors in
the defined order; |got_i - want_i| <= 4 G eps_R a_i and
| ||got||^2 - 1 | <= 8 G eps_R). Inputs are random dense states set with
set_state_vector and read back. Every case keeps |tau| sum|coeff| of one X/Y
mask at or below 1.
"""
import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import qrack_amd as qa
import pauli_oracle as po
import pauli_evolve_oracle as peo
import test_pauli_sum_gpu as psg

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(qa.hip_device_count() == 0, reason="no HIP device"),
]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("fp32", "fp64")
N12 = psg.N12


def hip_with_state(n, prec, seed):
    rng = np.random.default_rng(seed)
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=1)
    q.set_state_vector(po.random_state(n, rng, peo.DTYPE[prec]))
    return q, np.asarray(q.get_state_vector()), rng


@pytest.fixture(scope="module", params=PRECS)
def state12(request):
    """One random 12-qubit state per precision, downloaded once; sv never changes
    and every case uploads it again before it evolves the engine."""
    q, sv, _ = hip_with_state(N12, request.param, 1250)
    return request.param, q, sv


def check_rotation(q, sv, qs, ps, theta, prec):
    q.set_state_vector(sv)
    q.pauli_rotation(qs, ps, theta)
    want, a, gates = peo.rotate(sv, qs, ps, theta)
    peo.check(q.get_state_vector(), want, a, gates, prec, f"rot {qs} {ps}")


def check_sum(q, sv, terms, prec, steps=1, order=1, label="sum"):
    """evolve at the largest time the oracle's load limit allows"""
    time = steps / peo.group_load(terms, 1.0)
    assert peo.group_load(terms, time, steps) <= 1.0 + 1e-12
    q.set_state_vector(sv)
    q.evolve_pauli_sum(terms, time, steps, order)
    want, a, gates = peo.evolve(sv, terms, time, steps, order)
    got = np.asarray(q.get_state_vector())
    peo.check(got, want, a, gates, prec, label)
    return got


# ---- 1. index and partner logic ----------------------------------------------


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (1, 2, 5, 9))
def test_small_widths(n, prec):
    """Fewer pairs than a wave (1, 2, 5), fewer than a block and several blocks (9)."""
    q, sv, rng = hip_with_state(n, prec, 330 + n)
    if n <= 2:
        strings = [(list(range(n)), list(ps)) for ps in itertools.product(range(4), repeat=n)]
        terms = [(float(rng.uniform(-1, 1)), qs, ps) for qs, ps in strings]
    else:
        strings = [po.random_string(n, rng) for _ in range(48)]
        terms = po.random_terms(n, rng, 40)
    for qs, ps in strings:
        check_rotation(q, sv, qs, ps, float(rng.uniform(-1, 1)), prec)
    for order in (1, 2):
        check_sum(q, sv, terms, prec, steps=2, order=order, label=f"n{n} order{order}")


def partner_cases():
    """Per mask of psg.x_masks_12(): every string of strings_for_mask as a single
    rotation (qs, ps, theta), and all of them as one mixed re + im group."""
    out = []
    for x in psg.x_masks_12():
        rng = np.random.default_rng(7000 + x)
        strings = psg.strings_for_mask(x)
        rots = [(qs, ps, float(rng.uniform(-1, 1))) for qs, ps in strings]
        group = [(float(rng.uniform(-1, 1)), qs, ps) for qs, ps in strings]
        out.append((x, rots, group))
    return out


@pytest.mark.parametrize("case", partner_cases(), ids=lambda c: "x%03x" % c[0])
def test_partner_logic_12(state12, case):
    """bit 0 (in-vector swap, swapped back before the store), top bit, both,
    all bits, and single bits 5-8 (lane, wave and block boundaries of the pair
    stream), crossed with ny mod 4 and Z factors below and above the top x bit."""
    prec, q, sv = state12
    x, rots, group = case
    assert {po.masks(qs, ps)[0] for qs, ps, _ in rots} == {x}
    assert len({po.masks(qs, ps)[2] % 4 for qs, ps, _ in rots}) == min(4, bin(x).count("1") + 1)
    for qs, ps, theta in rots:
        check_rotation(q, sv, qs, ps, theta, prec)
    plan = qa.pauli_evolve_plan(group, N12, 1.0, 1, 1)
    assert len(plan) == 1 and [s for s, _ in plan[0][2]] == ["re", "im"]
    check_sum(q, sv, group, prec, label="group x%03x" % x)
    check_sum(q, sv, group, prec, steps=2, order=2, label="group x%03x order 2" % x)


# ---- 2. grouping ---------------------------------------------------------------


def one_parity_set(x, count, odd, rng):
    """count distinct strings with X/Y mask x whose Y count has the given parity"""
    xbits = [b for b in range(N12) if (x >> b) & 1]
    terms = []
    for z in rng.permutation(1 << N12):
        z = int(z)
        if (bin(x & z).count("1") & 1) != int(odd):
            continue
        qs, ps = [], []
        for b in range(N12):
            code = (1 if b in xbits else 0) | (2 if (z >> b) & 1 else 0)
            if code:
                qs.append(b)
                ps.append(code)
        terms.append((float(rng.uniform(-1, 1)), qs, ps))
        if len(terms) == count:
            break
    return terms


@pytest.mark.parametrize("x,odd", ((0, False), (0x212, False), (0x212, True)),
                         ids=("diag", "x212-re", "x212-im"))
def test_set_larger_than_cap_splits(state12, x, odd):
    """More terms in one commuting set than one launch holds: several launches
    of one planned pass. (A diagonal string has no Y factor, so no im set.)"""
    prec, q, sv = state12
    assert qa.PAULI_MAX_TERMS >= 1
    rng = np.random.default_rng(87)
    terms = one_parity_set(x, qa.PAULI_MAX_TERMS + 3, odd, rng)
    assert len(terms) == qa.PAULI_MAX_TERMS + 3
    plan = qa.pauli_evolve_plan(terms, N12, 1.0, 1, 1)
    assert len(plan) == 1 and [s for s, _ in plan[0][2]] == ["im" if odd else "re"]
    check_sum(q, sv, terms, prec, label="over the cap")


@pytest.mark.parametrize("order", (1, 2))
def test_mixed_sum_and_repeatability(state12, order):
    prec, q, sv = state12
    rng = np.random.default_rng(88)
    xs = [0] + [int(v) for v in rng.choice(np.arange(1, 1 << N12), size=9, replace=False)]
    terms = []
    for x in xs:
        terms += psg.terms_sharing_x(x, 10, rng)
    assert len(terms) == 100 and len({po.masks(qs, ps)[0] for _, qs, ps in terms}) == 10
    terms = [terms[i] for i in rng.permutation(len(terms))] + [(0.3, [], [])]
    got = check_sum(q, sv, terms, prec, steps=3, order=order, label=f"100 terms order {order}")
    other = qa.create_simulator(N12, engine="hip", precision=prec, seed=9)
    again = check_sum(other, sv, terms, prec, steps=3, order=order, label="second engine")
    assert got.tobytes() == again.tobytes()  # no atomics, no order dependence: bit-identical


# ---- 3. lazy basis state, tile sums ------------------------------------------------


@pytest.mark.parametrize("prec", PRECS)
def test_pending_basis_state(prec):
    n, p = 10, 0x2A5
    q = qa.create_simulator(n, engine="hip", precision=prec, seed=4)
    q.h(1)  # leave something else in the buffer first
    basis = np.zeros(1 << n, dtype=np.complex128)
    basis[p] = 1.0
    rng = np.random.default_rng(6)
    strings = [po.random_string(n, rng) for _ in range(8)]
    strings += [([3], [2]), ([0, 9, 4], [2, 2, 2]), ([], [])]  # x = 0: a pure phase
    assert sum(1 for qs, ps in strings if po.masks(qs, ps)[0] == 0) >= 3
    for qs, ps in strings:
        theta = float(rng.uniform(-1, 1))
        q.set_permutation(p)
        q.pauli_rotation(qs, ps, theta)
        want, a, gates = peo.rotate(basis, qs, ps, theta)
        peo.check(q.get_state_vector(), want, a, gates, prec, f"basis {qs} {ps}")


def test_tile_sums_dropped_by_rotation():
    """QFT leaves per-tile norms for the sampler. exp(-i pi/2 X) = -i X on the
    top qubit moves the weight between the halves of the state, so sampling
    from stale tile sums would show; it must match an engine that applied X."""
    n = 23
    pows = [1 << i for i in range(n)]

    def prepared():
        q = qa.create_simulator(n, engine="hip", seed=21)
        q.set_permutation(5)
        for i in range(0, n, 4):
            q.ry(0.9 + 0.05 * i, i)
        # The preparation of test_tile_sums_survive_pauli_sum alone leaves
        # prob(n-1) at 0.5. The transform's output is bit-reversed: input qubit
        # n-1 in cos(t/2)|0> + sin(t/2)|1> gives output qubit n-1 the
        # probability (1 - sin t) / 2, about 0.11 at t = 0.9.
        q.ry(0.9, n - 1)
        q.qft(0, n)
        return q

    a, b = prepared(), prepared()
    margin = abs(b.prob(n - 1) - 0.5)
    print("prob(n-1) =", b.prob(n - 1))
    assert margin > 0.1
    a.pauli_rotation([n - 1], [1], math.pi / 2)
    b.x(n - 1)
    shots_a = a.multi_shot_measure_mask(pows, 64)
    shots_b = b.multi_shot_measure_mask(pows, 64)
    assert sum(shots_a.values()) == 64
    assert shots_a == shots_b


# ---- 4. launch shape and streaming options: fresh child processes ---------------------


def child_partner_states(path):
    """run by the child: every partner-logic case on both precisions, states to `path`"""
    out = {}
    for prec in PRECS:
        q, sv, _ = hip_with_state(N12, prec, 1250)
        out[f"{prec}_sv"] = sv
        for x, rots, group in partner_cases():
            states = []
            for qs, ps, theta in rots:
                q.set_state_vector(sv)
                q.pauli_rotation(qs, ps, theta)
                states.append(np.asarray(q.get_state_vector()))
            q.set_state_vector(sv)
            q.evolve_pauli_sum(group, 1.0 / peo.group_load(group, 1.0))
            states.append(np.asarray(q.get_state_vector()))
            out[f"{prec}_{x}"] = np.stack(states)
    np.savez(path, **out)


def run_child(code, env, *args):
    r = subprocess.run(
        [sys.executable, "-c", code, ROOT, *args],
        env={**os.environ, **env}, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, f"stdout={r.stdout}\nstderr={r.stderr}"
    return r.stdout


_CHILD_STATES = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_pauli_evolve_gpu as t
t.child_partner_states(sys.argv[2])
print("CHILD_OK")
"""


@pytest.mark.parametrize("env", ({"QRACK_GPU_BLOCKS": "2"}, {"QRACK_GPU_NT": "1"}),
                         ids=("blocks2", "nontemporal"))
def test_env_variants_in_child(env, tmp_path):
    """QRACK_GPU_BLOCKS=2 leaves 512 threads for 1024 or more items, so the
    stride loop takes further trips; QRACK_GPU_NT=1 streams float4 with
    nontemporal loads and stores. Both are read once per process."""
    path = str(tmp_path / "states.npz")
    assert "CHILD_OK" in run_child(_CHILD_STATES, env, path)
    data = np.load(path)
    for prec in PRECS:
        sv = data[f"{prec}_sv"]
        for x, rots, group in partner_cases():
            states = data[f"{prec}_{x}"]
            assert len(states) == len(rots) + 1
            for got, (qs, ps, theta) in zip(states, rots):
                want, a, gates = peo.rotate(sv, qs, ps, theta)
                peo.check(got, want, a, gates, prec, f"child rot {qs} {ps}")
            want, a, gates = peo.evolve(sv, group, 1.0 / peo.group_load(group, 1.0))
            peo.check(states[-1], want, a, gates, prec, "child group x%03x" % x)


# ---- 5. pass counts, through the layers ---------------------------------------------------

N_PROF = 13  # the hybrid layer hands its state to the HIP engine from 13 qubits on


def heisenberg(n):
    terms = []
    for b in range(n - 1):
        terms += [(1.0, [b, b + 1], [1, 1]), (0.8, [b, b + 1], [3, 3]), (0.6, [b, b + 1], [2, 2])]
    return terms


def child_profile():
    """run by the child under QRACK_PROFILE=1: pass counts per stack as JSON"""
    terms = heisenberg(N_PROF)
    report = {}
    bare = None
    for name, kw in (("hip", dict(engine="hip")), ("hybrid", dict(layers=["hybrid"])),
                     ("fuser-hip", dict(layers=["fuser", "hip"]))):
        counts = {}
        for order, steps in ((1, 1), (2, 3)):
            q = qa.create_simulator(N_PROF, seed=3, **kw)
            for i in range(N_PROF):
                q.ry(0.2 + 0.3 * i, i)
            for i in range(N_PROF - 1):
                q.cnot(i, i + 1)
            q.get_state_vector()  # the fuser has flushed before the counters restart
            qa.profile_reset()
            q.evolve_pauli_sum(terms, 0.3, steps, order)
            rep = qa.profile_report()
            counts[f"order{order}"] = {k: int(v[0]) for k, v in rep.items()}
            q.pauli_rotation([0, 5], [3, 1], 0.4)
            state = np.asarray(q.get_state_vector())
        if bare is None:
            bare = state
        report[name] = {"counts": counts, "maxdiff": float(np.abs(state - bare).max())}
    print("REPORT " + json.dumps(report))


_CHILD_PROFILE = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_pauli_evolve_gpu as t
t.child_profile()
"""


@pytest.fixture(scope="module")
def profile_report():
    out = run_child(_CHILD_PROFILE, {"QRACK_PROFILE": "1"})
    line = [l for l in out.splitlines() if l.startswith("REPORT ")][-1]
    return json.loads(line[len("REPORT "):])


def planned(order, steps):
    return len(qa.pauli_evolve_plan(heisenberg(N_PROF), N_PROF, 0.3, steps, order))


def test_profile_counts_the_planned_passes(profile_report):
    assert planned(1, 1) == N_PROF
    assert planned(2, 3) == 3 * (2 * N_PROF - 1) - 2
    counts = profile_report["hip"]["counts"]
    # nothing but the evolution passes ran: no gate-path op is counted
    assert counts["order1"] == {"pauli_evolve": planned(1, 1)}
    assert counts["order2"] == {"pauli_evolve": planned(2, 3)}


@pytest.mark.parametrize("stack", ("hybrid", "fuser-hip"))
def test_layers_reach_engine(profile_report, stack):
    counts = profile_report[stack]["counts"]
    assert counts["order1"] == {"pauli_evolve": planned(1, 1)}
    assert counts["order2"] == {"pauli_evolve": planned(2, 3)}
    # the same kernels on the same amplitudes as the bare engine
    assert profile_report[stack]["maxdiff"] <= 2e-4
