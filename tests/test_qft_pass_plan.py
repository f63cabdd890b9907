"""qft_pass_plan: the HIP engine's QFT schedule as a pure host function.

A plan is a list of (kind, colLo, nCols), top pass first: "low" is the low
ladder through contiguous LDS tiles, "mid" a 2D-tile pass (2/3/4/6 columns
on the 64-amplitude-run kernel, 8/9 on the wide-tile one), "col" 1..4
columns fused in registers. midmax=6 must be the six-at-a-time schedule the
engine took before the planner existed; it is written out below, derived
by hand from those branches (tile bits 12 / 11, ladder K 4 / 3, at most
four fused register columns, mid passes fp32 only).
"""
import pytest

import qrack_amd as qa

TILE_BITS = {"fp32": 12, "fp64": 11}
LADDER_K = {"fp32": 4, "fp64": 3}
WIDE_LOWBITS = 4

# "m17.6" = mid pass, colLo 17, 6 columns; "c8.3" = 3 register columns from
# column 8; "l8" = low ladder over columns 7..0. Full-width registers.
SIX_AT_A_TIME = {
    "fp32": {
        1: "c0.1",
        2: "c1.1 c0.1",
        3: "c1.2 c0.1",
        4: "c1.3 c0.1",
        5: "c1.4 c0.1",
        6: "c2.4 c0.2",
        7: "c3.4 c0.3",
        8: "c4.4 c0.4",
        9: "c5.4 c1.4 c0.1",
        10: "c6.4 c2.4 c0.2",
        11: "c7.4 c3.4 c0.3",
        12: "l12",
        13: "c9.4 c8.1 l8",
        14: "m12.2 l12",
        15: "m12.3 l12",
        16: "m12.4 l12",
        17: "m11.6 c8.3 l8",
        18: "m12.6 l12",
        19: "m13.6 c9.4 c8.1 l8",
        20: "m14.6 m12.2 l12",
        21: "m15.6 m12.3 l12",
        22: "m16.6 m12.4 l12",
        23: "m17.6 m11.6 c8.3 l8",
        24: "m18.6 m12.6 l12",
        25: "m19.6 m13.6 c9.4 c8.1 l8",
        26: "m20.6 m14.6 m12.2 l12",
        27: "m21.6 m15.6 m12.3 l12",
        28: "m22.6 m16.6 m12.4 l12",
        29: "m23.6 m17.6 m11.6 c8.3 l8",
        30: "m24.6 m18.6 m12.6 l12",
        31: "m25.6 m19.6 m13.6 c9.4 c8.1 l8",
        32: "m26.6 m20.6 m14.6 m12.2 l12",
        33: "m27.6 m21.6 m15.6 m12.3 l12",
        34: "m28.6 m22.6 m16.6 m12.4 l12",
    },
    "fp64": {
        1: "c0.1",
        2: "c1.1 c0.1",
        3: "c1.2 c0.1",
        4: "c1.3 c0.1",
        5: "c1.4 c0.1",
        6: "c2.4 c0.2",
        7: "c3.4 c0.3",
        8: "c4.4 c0.4",
        9: "c5.4 c1.4 c0.1",
        10: "c6.4 c2.4 c0.2",
        11: "c9.2 l9",
        12: "c8.4 c6.2 l6",
        13: "c9.4 l9",
        14: "c10.4 c9.1 l9",
        15: "c11.4 c9.2 l9",
        16: "c12.4 c8.4 c6.2 l6",
        17: "c13.4 c9.4 l9",
        18: "c14.4 c10.4 c9.1 l9",
        19: "c15.4 c11.4 c9.2 l9",
        20: "c16.4 c12.4 c8.4 c6.2 l6",
        21: "c17.4 c13.4 c9.4 l9",
        22: "c18.4 c14.4 c10.4 c9.1 l9",
        23: "c19.4 c15.4 c11.4 c9.2 l9",
        24: "c20.4 c16.4 c12.4 c8.4 c6.2 l6",
        25: "c21.4 c17.4 c13.4 c9.4 l9",
        26: "c22.4 c18.4 c14.4 c10.4 c9.1 l9",
        27: "c23.4 c19.4 c15.4 c11.4 c9.2 l9",
        28: "c24.4 c20.4 c16.4 c12.4 c8.4 c6.2 l6",
        29: "c25.4 c21.4 c17.4 c13.4 c9.4 l9",
        30: "c26.4 c22.4 c18.4 c14.4 c10.4 c9.1 l9",
        31: "c27.4 c23.4 c19.4 c15.4 c11.4 c9.2 l9",
        32: "c28.4 c24.4 c20.4 c16.4 c12.4 c8.4 c6.2 l6",
        33: "c29.4 c25.4 c21.4 c17.4 c13.4 c9.4 l9",
        34: "c30.4 c26.4 c22.4 c18.4 c14.4 c10.4 c9.1 l9",
    },
}

PRECISIONS = ("fp32", "fp64")
LENGTHS = range(1, 35)
# (length, width): full-width registers and a few shorter than the engine
SHAPES = [(n, n) for n in LENGTHS] + [(21, 23), (20, 24), (13, 30), (30, 34), (12, 20), (5, 16)]


def parse(text):
    kinds = {"l": "low", "m": "mid", "c": "col"}
    plan = []
    for tok in text.split():
        if tok[0] == "l":
            plan.append(("low", 0, int(tok[1:])))
        else:
            lo, nc = tok[1:].split(".")
            plan.append((kinds[tok[0]], int(lo), int(nc)))
    return plan


def plan(length, width, precision, midmax=None):
    got = (qa.qft_pass_plan(length, width, precision) if midmax is None
           else qa.qft_pass_plan(length, width, precision, midmax))
    return [tuple(p) for p in got]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_midmax_6_is_the_six_at_a_time_schedule(precision):
    for n in LENGTHS:
        assert plan(n, n, precision, 6) == parse(SIX_AT_A_TIME[precision][n]), (precision, n)


def test_midmax_7_and_below_leave_the_six_at_a_time_schedule():
    for n in LENGTHS:
        for midmax in (0, 4, 7):
            assert plan(n, n, "fp32", midmax) == plan(n, n, "fp32", 6)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_default_is_midmax_9_and_never_takes_more_passes(precision):
    for length, width in SHAPES:
        wide = plan(length, width, precision)
        assert wide == plan(length, width, precision, 9)
        assert len(wide) <= len(plan(length, width, precision, 6)), (length, width)


def test_fp64_is_unchanged():
    for length, width in SHAPES:
        assert plan(length, width, "fp64") == plan(length, width, "fp64", 6)


def test_30_qubits_fp32_is_three_passes():
    assert plan(30, 30, "fp32") == [("mid", 21, 9), ("mid", 12, 9), ("low", 0, 12)]


def test_wide_schedules():
    assert plan(20, 20, "fp32") == [("mid", 12, 8), ("low", 0, 12)]
    assert plan(21, 21, "fp32") == [("mid", 12, 9), ("low", 0, 12)]
    assert plan(21, 23, "fp32") == [("mid", 12, 9), ("low", 0, 12)]
    assert plan(25, 25, "fp32") == [("mid", 16, 9), ("mid", 12, 4), ("low", 0, 12)]
    assert plan(27, 27, "fp32") == [("mid", 18, 9), ("mid", 12, 6), ("low", 0, 12)]
    assert len(plan(23, 23, "fp32")) == 3
    assert len(plan(34, 34, "fp32")) == 4
    assert plan(34, 34, "fp32", 8) == [
        ("mid", 26, 8), ("mid", 18, 8), ("mid", 12, 6), ("low", 0, 12)]


def test_a_tie_keeps_the_64_wide_kernel():
    # 22 = 6 + 4 + 12 and 22 = 9 + 9 + 4 are both three passes
    assert plan(22, 22, "fp32") == parse(SIX_AT_A_TIME["fp32"][22])
    # no wide pass can shorten these either
    for n in (14, 15, 16, 18, 24):
        assert plan(n, n, "fp32") == parse(SIX_AT_A_TIME["fp32"][n])


@pytest.mark.parametrize("midmax", (6, 8, 9))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_plan_is_well_formed(precision, midmax):
    tb, k = TILE_BITS[precision], LADDER_K[precision]
    for length, width in SHAPES:
        passes = plan(length, width, precision, midmax)
        # columns length-1..0 exactly once, top-down
        top = length
        for kind, lo, nc in passes:
            assert nc >= 1 and lo + nc == top, (length, width, passes)
            top = lo
        assert top == 0
        for idx, (kind, lo, nc) in enumerate(passes):
            if kind == "low":
                assert idx == len(passes) - 1 and lo == 0
                assert nc % k == 0 and nc <= tb and width >= tb
            elif kind == "mid":
                assert precision == "fp32" and width >= tb
                assert lo + nc > tb  # its top column is above the low tile
                if nc in (2, 3, 4, 6):
                    assert lo >= 6
                else:
                    assert nc in (8, 9) and nc <= midmax and lo >= WIDE_LOWBITS
            else:
                assert kind == "col" and nc <= 4 and (nc == 1 or width >= nc + 1)


def test_rejects_bad_arguments():
    with pytest.raises(ValueError):
        qa.qft_pass_plan(5, 4, "fp32")
    with pytest.raises(ValueError):
        qa.qft_pass_plan(5, 5, "fp16")
    assert plan(0, 5, "fp32") == []
