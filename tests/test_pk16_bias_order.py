"""Why the biased packed score pass (exonerate_amd/csrc/c4_viterbi16_kernel.h, BIAS) may take a three-way integer maximum through
v_pk_maximum3_f16: on the bit patterns its guard lets in, the IEEE half order is the integer order.  numpy only; the constants
are read from exonerate_amd/csrc/c4_pk16_bias.h."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "exonerate_amd", "csrc", "c4_pk16_bias.h")).read()


def const(name):
    m = re.search(r"constexpr int %s = (0x[0-9A-Fa-f]+|\d+);" % name, HEADER)
    assert m, name
    return int(m.group(1), 0)


G = const("PK16_SCORE_MAX")
FINITE_MAX = const("PK16_HALF_FINITE_MAX")
NORMAL_MIN = const("PK16_HALF_NORMAL_MIN")
POST = const("PK16_POST_GAIN_MAX")
B = FINITE_MAX - G - POST                # PK16_BIAS, as the header derives it
A = (B - NORMAL_MIN) // 2                # PK16_ADDEND_MAX


def halves(ints):
    """int16 values as the float16 their bit patterns are"""
    return np.asarray(ints, dtype=np.int16).view(np.float16)


def test_header_derives_the_constants_this_way():
    assert re.search(r"PK16_BIAS = PK16_HALF_FINITE_MAX - PK16_SCORE_MAX - PK16_POST_GAIN_MAX;", HEADER)
    assert re.search(r"PK16_ADDEND_MAX = \(PK16_BIAS - PK16_HALF_NORMAL_MIN\) / 2;", HEADER)
    assert (G, FINITE_MAX, NORMAL_MIN) == (16000, 0x7BFF, 0x0400)
    assert B <= 15743 and B + G <= FINITE_MAX                    # the largest legitimate half is finite
    assert 2 * A + NORMAL_MIN <= B                               # the smallest legitimate candidate is a normal half
    assert FINITE_MAX - 32768 == -1025                           # a dead row: legitimate + (-32 768) is at most 0xFBFF ...
    assert np.isfinite(halves([-1025])[0]) and halves([-1025])[0] < 0
    assert -32768 + G + POST < -1024                             # ... and so is the lineage of `unset`


def test_non_negative_finite_halves_are_strictly_increasing():
    f = halves(np.arange(0, FINITE_MAX + 1)).astype(np.float64)
    assert len(f) == 31744 and np.all(np.isfinite(f)) and np.all(np.diff(f) > 0) and f[0] == 0.0


def test_garbage_band_is_finite_and_negative():
    f = halves(np.arange(-32768, -32768 + G + POST + 1)).astype(np.float64)
    assert np.all(np.isfinite(f)) and np.all(f <= 0) and np.all(np.signbit(f))
    assert np.all(f[1:] < 0)                                     # 0x8000 itself is -0.0


def test_excluded_bands_are_exactly_nan_and_inf():
    allv = np.arange(-32768, 32768)
    bad = ~np.isfinite(halves(allv).astype(np.float64))
    excluded = ((allv >= -1024) & (allv <= -1)) | ((allv >= 31744) & (allv <= 32767))
    assert np.array_equal(bad, excluded)


def test_three_way_float_maximum_is_the_integer_maximum():
    rng = np.random.default_rng(20260119)
    n = 100000
    legit = lambda: rng.integers(B - 2 * A, B + G + 1, n)
    garbage = lambda: rng.integers(-32768, -32768 + G + POST + 1, n)
    dead = lambda: rng.integers(B - 2 * A, B + G + 1, n) - 32768        # legitimate + an addend of exactly -32 768
    for kinds in ((legit, legit, legit), (legit, garbage, legit), (garbage, legit, garbage), (legit, dead, garbage),
                  (dead, dead, legit)):
        x, y, z = (k() for k in kinds)
        want = np.maximum(np.maximum(x, y), z)
        got = np.maximum(np.maximum(halves(x), halves(y)), halves(z)).view(np.int16).astype(np.int64)
        assert np.array_equal(got, want)
    # the edges of the legitimate band
    x = np.array([B - 2 * A, NORMAL_MIN, B + G, FINITE_MAX, B, B])
    y = np.array([-32768, -1025, -32768 + G, -1025, B - 1, B + 1])
    assert np.array_equal(np.maximum(halves(x), halves(y)).view(np.int16), np.maximum(x, y).astype(np.int16))


def test_operand_from_an_excluded_band_is_not_covered():
    # why the host's guard exists: -1 is a NaN pattern and poisons the maximum, 32 000 is one too, and the integer maximum of
    # (legitimate, -1) is the legitimate value
    for bad in (-1, -1023, 31745, 32767):
        got = np.maximum(halves([B + 100]), halves([bad]))
        assert np.isnan(got[0]), bad
    # (the bands' other ends are the infinities: +inf wins where the integer 31 744 would too, -inf loses: kept out with the NaNs)
    assert np.isinf(halves([31744, -1024])).all()
    # an addend just past the guard's limit takes the lowest candidate the guard allows below the normal halves' floor ...
    assert B - 2 * (A + 1) < NORMAL_MIN
    # ... and one in the unsafe band takes a legitimate value into the NaN band
    assert -1024 <= (B + 100) - (B + 101) <= -1
