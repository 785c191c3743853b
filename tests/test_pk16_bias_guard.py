"""The host's guard of the biased packed score pass (exonerate_amd/csrc/c4_pk16_bias.h: pk16_bias_fits) at its edges, and the
kernel a launch gets when the guard refuses (c4_kernel_choice.h: LaunchFacts::pk16_bias_unfit), on the host through
tests/pk16_bias_sim.hip."""
import pytest

import pk16_bias_sim_lib as pb

# est2genome's defaults: match 5 / mismatch -4 (N: 0), gap open -12, extend -4, intron penalty -30; a site's worst sum is a few
# dozen below zero, its best 16
SUBMAT = [5 if a == b else -4 for a in range(4) for b in range(4)] + [0] * 8
CALCS = [0, -12, -4, -30, 0, -30, 0]
WORST = [-30 - 60, -60, -30 - 60, -60]
BEST = 16


def test_constants_are_consistent():
    c = pb.constants()
    assert c["bias"] + c["score_max"] + c["post_gain_max"] <= 0x7BFF
    assert 2 * c["addend_max"] + 0x0400 <= c["bias"] < 2 * (c["addend_max"] + 1) + 0x0400


def test_default_parameters_fit():
    assert pb.fits(SUBMAT, CALCS, WORST, BEST)


@pytest.mark.parametrize("where", ["gap open", "mismatch", "calc"])
def test_largest_negative_addend(where):
    a = pb.constants()["addend_max"]
    for value, ok in ((-a, True), (-a - 1, False), (-32767, False), (-32768, True), (a + 1, True)):
        sub, calcs = list(SUBMAT), list(CALCS)
        if where == "gap open":
            calcs[1] = value
        elif where == "mismatch":
            sub[1] = value
        else:
            calcs[-1] = value
        assert pb.fits(sub, calcs, WORST, BEST) == ok, (where, value)


def test_forcegtag_sentinel_is_allowed():
    # a site that is not GT / AG scores -987 654 321 in its sum's place (with the pre-splice constant folded in or not): as a splice
    # value the kernel receives it clamps to exactly -32 768, which the biased form carries
    assert pb.addend_ok(-987654321) and pb.addend_ok(-987654321 - 30) and pb.addend_ok(-32768)
    assert not pb.addend_ok(-32767)
    # ... but a site's worst PSSM SUM that low says nothing about the sums between: a sum passes by its magnitude alone
    a = pb.constants()["addend_max"]
    assert pb.site_ok(-a) and not pb.site_ok(-a - 1) and not pb.site_ok(-32768) and not pb.site_ok(-987654321)
    assert not pb.fits(SUBMAT, CALCS, [-40000, -60, -90, -60], BEST)


def test_worst_site_sum_inside_and_outside():
    a = pb.constants()["addend_max"]
    for k in range(4):
        inside, outside = list(WORST), list(WORST)
        inside[k], outside[k] = -a, -a - 1
        assert pb.fits(SUBMAT, CALCS, inside, BEST) and not pb.fits(SUBMAT, CALCS, outside, BEST)


def test_post_splice_gain_inside_and_outside():
    g = pb.constants()["post_gain_max"]
    assert pb.fits(SUBMAT, CALCS, WORST, g) and not pb.fits(SUBMAT, CALCS, WORST, g + 1)


@pytest.mark.parametrize("qlen, n, fit_kernel", [(1000, 4096, "kpk16f"), (300, 64, "kpk16g"), (1030, 4096, "kpk16h"),
                                                  (1600, 4096, "kpk16j")])
def test_choice_when_the_guard_refuses(qlen, n, fit_kernel):
    assert pb.choose(qlen, n, False) == (fit_kernel + "_est2genome", {"fmt16", "needs_ss16", "staged_codes"})
    # the form that loads per step, with 16-bit dumps and the packed splice array, and no residue-code table
    assert pb.choose(qlen, n, True) == ("kpk16d_est2genome", {"fmt16", "needs_ss16"})
