"""qft_sparse_last_plan: which 16-point orbits of the last low-ladder pass of
a QFT of |perm> hold a nonzero input, and where.

Entering the last pass a tile is nonzero only where the in-tile index agrees
with perm in the ladder's n_cols low bits. The schedule names, per K=4 orbit
group, the `below` value of the orbits that contain such an amplitude, how
many there are per tile, and the slot of the orbit the amplitude sits in.
Here it is compared with a brute-force propagation of the support through
the groups.
"""
import numpy as np
import pytest

import qrack_amd as qa

TB = 12
K = 4
TILE = 1 << TB
PERMS = (0, 0xFFF, 0x00F, 0x0F0, 0xF00, 0xA5A, 0x5A5A5A5A, 1, 1 << 29, 0x123456789)


def brute_force(n_cols, perm):
    """[(g_lo, real orbits, set of their below values, set of nonzero slots)]
    for the groups in execution order, from a 4096-entry support vector."""
    j = np.arange(TILE)
    support = ((j ^ (perm & (TILE - 1))) & ((1 << n_cols) - 1)) == 0
    out = []
    for g_lo in range(n_cols - K, -1, -K):
        belows, slots, real = set(), set(), 0
        after = support.copy()
        for o in range(TILE >> K):
            below = o & ((1 << g_lo) - 1)
            r = ((o >> g_lo) << (g_lo + K)) | below
            pos = r | (np.arange(1 << K) << g_lo)
            hit = np.nonzero(support[pos])[0]
            if hit.size:
                real += 1
                belows.add(below)
                slots.update(int(b) for b in hit)
                after[pos] = True
        support = after
        out.append((g_lo, real, belows, slots))
    assert support.all()  # the last group fills the tile
    return out


@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("n_cols", (8, 12))
def test_schedule_matches_the_propagated_support(n_cols, perm):
    plan = qa.qft_sparse_last_plan(n_cols, perm)
    assert plan["eligible"]
    ref = brute_force(n_cols, perm)
    assert [g["g_lo"] for g in plan["groups"]] == [r[0] for r in ref]
    for g, (g_lo, real, belows, slots) in zip(plan["groups"], ref):
        assert g["real_orbits"] == real, (g_lo, g, real)
        assert belows == {g["below"]}, (g_lo, g, belows)
        assert slots == {g["slot"]}, (g_lo, g, slots)


def test_group_counts():
    assert [g["real_orbits"] for g in qa.qft_sparse_last_plan(12, 0xA5A)["groups"]] == [1, 16, 256]
    assert [g["real_orbits"] for g in qa.qft_sparse_last_plan(8, 0xA5A)["groups"]] == [16, 256]
    assert [g["g_lo"] for g in qa.qft_sparse_last_plan(12, 0)["groups"]] == [8, 4, 0]
    assert [g["g_lo"] for g in qa.qft_sparse_last_plan(8, 0)["groups"]] == [4, 0]


def test_real_slot_and_below_spell_the_permutation():
    for n_cols in (8, 12):
        for perm in PERMS:
            for g in qa.qft_sparse_last_plan(n_cols, perm)["groups"]:
                low = perm & ((1 << (g["g_lo"] + K)) - 1)
                assert g["below"] | (g["slot"] << g["g_lo"]) == low


@pytest.mark.parametrize("n_cols", (0, 4, 6, 9, 16))
def test_other_ladders_are_not_eligible(n_cols):
    plan = qa.qft_sparse_last_plan(n_cols, 5)
    assert not plan["eligible"]
    assert plan["groups"] == []
