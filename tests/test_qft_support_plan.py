"""qft_support_plan: the support-restricted schedule of a QFT/IQFT applied to
a basis state, as a pure host function.

A QFT column is an H and a phase ladder controlled by lower bits, so phase*|p>
stays a product state: after the columns F ("free" bits) an amplitude x is
nonzero only where ((x ^ p) & ~F) == 0. Each pass reports

  fixed_mask   ~F on entry (input nonzero only where ((x ^ p) & fixed_mask) == 0)
  from_buffer  F non-empty: the in-support input is loaded, else it is the phase
  tile_free    the tile-index bits the pass counts through
  tile_fixed   the value of the other tile-index bits
  active_tiles 2^popcount(tile_free)

Every pass but the last writes its active tiles whole and the buffer holds
nothing defined anywhere else, so what a pass reads must lie inside what the
pass before wrote, and the last pass must visit every tile. Both are checked
here for every eligible width, by enumeration where the state is small and
through the bit masks at every width.
"""
import numpy as np
import pytest

import qrack_amd as qa

WIDE_LB = 4
TB = 12


def support(width, perm=0, inverse=False, length=None, precision="fp32"):
    return qa.qft_support_plan(width if length is None else length, width, precision, perm, inverse)


def perms_for(width):
    mask = (1 << width) - 1
    return (0, mask, 0x5A5A5A5A & mask, 1 << (width - 1), 1, 0x2B3C4D5E6F & mask)


@pytest.mark.parametrize("width,inverse,want", [
    (30, False, [1, 512, 262144]),
    (30, True, [1, 256, 131072]),
    (22, False, [1, 64, 1024]),
    (17, False, [1, 32]),
])
def test_active_tile_counts(width, inverse, want):
    for perm in perms_for(width):
        sp = support(width, perm, inverse)
        assert sp["eligible"]
        assert [p["active_tiles"] for p in sp["passes"]] == want


def test_pass_lists_follow_the_pass_plan():
    assert [(p["kind"], p["col_lo"], p["n_cols"]) for p in support(22)["passes"]] == [
        ("mid", 16, 6), ("mid", 12, 4), ("low", 0, 12)]
    assert [(p["kind"], p["col_lo"], p["n_cols"]) for p in support(17)["passes"]] == [
        ("mid", 8, 9), ("low", 0, 8)]
    for width in range(14, 35):
        fwd = [tuple(p) for p in qa.qft_pass_plan(width, width, "fp32")]
        for inverse in (False, True):
            sp = support(width, 5, inverse)
            got = [(p["kind"], p["col_lo"], p["n_cols"]) for p in sp["passes"]]
            if sp["eligible"]:
                assert got == (fwd[::-1] if inverse else fwd)
            else:
                assert got == []


@pytest.mark.parametrize("inverse", [False, True])
def test_not_eligible(inverse):
    for width in (12, 13, 19):  # one pass, or a plan with a register-column pass
        assert not support(width, 3, inverse)["eligible"]
    for width in range(1, 35):
        assert not support(width, 0, inverse, precision="fp64")["eligible"]
    for width, length in ((22, 21), (23, 21), (30, 29), (20, 14)):
        assert not support(width, 1, inverse, length=length)["eligible"]


def test_eligible_widths():
    eligible = [w for w in range(1, 36) if support(w)["eligible"]]
    assert eligible == [14, 15, 16, 17, 18] + list(range(20, 36))
    for w in eligible:
        assert support(w, 0, True)["eligible"]


def test_rejects_bad_arguments():
    with pytest.raises(ValueError):
        qa.qft_support_plan(5, 4, "fp32")
    with pytest.raises(ValueError):
        qa.qft_support_plan(5, 5, "fp16")


# ---- the geometry of a pass, restated here independently ----------------------


def tile_geometry(p):
    """(low_bits, in-tile x-bit mask) of a pass."""
    if p["kind"] == "low":
        return TB, (1 << TB) - 1
    lb = WIDE_LB if p["n_cols"] >= 8 else 6
    return lb, ((1 << lb) - 1) | (((1 << p["n_cols"]) - 1) << p["col_lo"])


def tile_index(x, p):
    lb, _ = tile_geometry(p)
    if p["kind"] == "low":
        return x >> lb
    mid = (1 << (p["col_lo"] - lb)) - 1
    return ((x >> (p["col_lo"] + p["n_cols"])) << (p["col_lo"] - lb)) | ((x >> lb) & mid)


def x_bits_of_tile_bits(tmask, p, width):
    """x-bit mask whose tile-index image is tmask."""
    out = 0
    for b in range(width):
        if tile_index(1 << b, p) & tmask:
            out |= 1 << b
    return out


def eligible_cases():
    return [(w, inv) for w in range(14, 35) for inv in (False, True)
            if support(w, 0, inv)["eligible"]]


@pytest.mark.parametrize("width,inverse", eligible_cases())
def test_masks_cover_and_chain(width, inverse):
    """Through the masks, at every width: the written set of a pass is
    {x : ((x ^ p) & wfix) == 0}, the read set {x : ((x ^ p) & rfix) == 0};
    read within written means wfix is a subset of rfix."""
    all_bits = (1 << width) - 1
    for perm in perms_for(width):
        sp = support(width, perm, inverse)
        free = 0
        prev_wfix = None
        n = len(sp["passes"])
        for k, p in enumerate(sp["passes"]):
            lb, in_tile = tile_geometry(p)
            cols = ((1 << p["n_cols"]) - 1) << p["col_lo"]
            assert p["low_bits"] == lb
            assert p["tile_index_bits"] == width - bin(in_tile).count("1")
            n_tiles = 1 << p["tile_index_bits"]
            assert p["fixed_mask"] == all_bits & ~free
            assert p["from_buffer"] == (free != 0)
            assert p["tile_free"] & p["tile_fixed"] == 0
            assert (p["tile_free"] | p["tile_fixed"]) < n_tiles
            assert p["active_tiles"] == 1 << bin(p["tile_free"]).count("1")
            if k == n - 1:
                assert p["tile_free"] == n_tiles - 1 and p["tile_fixed"] == 0
                assert p["active_tiles"] == n_tiles
            else:
                # exactly the tiles that can hold a nonzero amplitude
                assert p["tile_free"] == tile_index(free, p) & (n_tiles - 1)
                # the other tile-index bits hold p's values
                assert p["tile_fixed"] == tile_index(perm, p) & ~p["tile_free"]
            tile_fixed_x = x_bits_of_tile_bits((n_tiles - 1) & ~p["tile_free"], p, width)
            assert tile_fixed_x & in_tile == 0
            wfix = tile_fixed_x  # the pass writes its active tiles whole
            rfix = tile_fixed_x | p["fixed_mask"]
            if k == 0:
                assert not p["from_buffer"]  # nothing is read at all
            else:
                assert prev_wfix & ~rfix == 0, "reads outside what the previous pass wrote"
            # the support after the pass lies inside what it wrote
            free |= cols
            assert wfix & free == 0
            prev_wfix = wfix
        assert free == all_bits


@pytest.mark.parametrize("width,inverse", [c for c in eligible_cases() if c[0] <= 20])
def test_read_sets_inside_write_sets_by_enumeration(width, inverse):
    x = np.arange(1 << width, dtype=np.int64)
    for perm in (0x5A5A5A5A & ((1 << width) - 1), 1 << (width - 1)):
        sp = support(width, perm, inverse)
        written = None
        for k, p in enumerate(sp["passes"]):
            t = np.array(tile_index(x, p))
            active = (t & ~np.int64(p["tile_free"])) == p["tile_fixed"]
            assert np.unique(t[active]).size == p["active_tiles"]
            in_support = ((x ^ perm) & p["fixed_mask"]) == 0
            if p["from_buffer"]:
                reads = active & in_support
                assert not np.any(reads & ~written)
            else:
                assert k == 0
            # a nonzero input can only sit in an active tile
            assert not np.any(in_support & ~active)
            written = active
        assert written.all()
