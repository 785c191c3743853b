// c4_pk16_bias.h — the constants of the biased form of the packed score pass (c4_viterbi16_kernel.h, BIAS) and the host's
// guard for it, as pure functions of plain data: compiled into the kernels, the engine and tests/pk16_bias_sim.hip alike.
//
// The biased form carries every score half as real + PK16_BIAS, so that the halves a result depends on are bit patterns of
// non-negative NORMAL IEEE halves, [0x0400, 0x7BFF]: there the float order is the integer order, and one v_pk_maximum3_f16 is a
// three-way integer maximum.  What must never enter such a maximum is a NaN or infinity pattern: as int16, [-1024, -1] and
// [31744, 32767].
#pragma once

namespace c4k {

constexpr int PK16_SCORE_MAX = 16000;            // Engine::pk16_fits: no real score a result depends on exceeds it
constexpr int PK16_HALF_FINITE_MAX = 0x7BFF;     // 65 504, the largest finite half: 31 743 as int16
constexpr int PK16_HALF_NORMAL_MIN = 0x0400;     // the smallest normal half: below it the FP16 denormal mode could matter
// An intron entered through a site that scores exactly -32 768 (--forcegtag's sentinel, clamped) holds legitimate - 32 768; the
// post-splice transition out of it may ADD a site's score before the value enters a match state's maximum, and the sum must
// still be a negative finite half, <= -1 025: the bias leaves room for a post-splice site of up to this much (default
// parameters: 16; the guard checks it)
constexpr int PK16_POST_GAIN_MAX = 127;
constexpr int PK16_BIAS = PK16_HALF_FINITE_MAX - PK16_SCORE_MAX - PK16_POST_GAIN_MAX;       // 15 616
// the largest magnitude A of a negative addend: a candidate of a match state is at most two of them below START's PK16_BIAS
constexpr int PK16_ADDEND_MAX = (PK16_BIAS - PK16_HALF_NORMAL_MIN) / 2;                      // 7 296
static_assert(PK16_BIAS + PK16_SCORE_MAX + PK16_POST_GAIN_MAX <= PK16_HALF_FINITE_MAX, "the largest legitimate half is finite");
static_assert(PK16_BIAS - 2 * PK16_ADDEND_MAX >= PK16_HALF_NORMAL_MIN, "the smallest legitimate candidate is a normal half");
static_assert(PK16_HALF_FINITE_MAX - 32768 == -1025 && -1025 < -1024, "legitimate + (-32 768) is a negative finite half (0xFBFF at most)");
static_assert(-32768 + PK16_SCORE_MAX + PK16_POST_GAIN_MAX < -1024, "the lineage of `unset` stays a negative finite half");

// One addend as the model has it, before the kernel clamps it to 16 bits.  Safe: nothing negative (a legitimate sum stays
// legitimate), at most PK16_ADDEND_MAX in magnitude, or so low that it clamps to EXACTLY -32 768 (-987 654 321: legitimate +
// (-32 768) <= -1 025).  Anything between takes a legitimate half into or past the NaN band.
inline bool pk16_bias_addend_ok(long long v) { return v >= -(long long)PK16_ADDEND_MAX || v <= -32768; }

// A site's sum is a SUM: that its worst lies below -32 768 says nothing about the sums between, so a worst sum passes only by its
// magnitude.  (--forcegtag's -987 654 321 is no PSSM sum: the splice predictor writes it in the sum's place, and the kernel's
// clamp takes it to exactly -32 768, which the biased form carries.)
inline bool pk16_bias_site_ok(long long worst_sum) { return worst_sum >= -(long long)PK16_ADDEND_MAX; }

// The guard: the substitution scores of the launch, the calc constants, the WORST sums of the four splice sites as the packed
// pass adds them (the pre-splice calc constant folded in: ss16_kernel), and the best sum a post-splice site can add.
inline bool pk16_bias_fits(const int *submat, int n_submat, const int *calc_value, int n_calcs, const long long *site_worst,
                           int n_sites, long long post_best) {
    for (int i = 0; i < n_submat; i++) if (!pk16_bias_addend_ok(submat[i])) return false;
    for (int i = 0; i < n_calcs; i++) if (!pk16_bias_addend_ok(calc_value[i])) return false;
    for (int i = 0; i < n_sites; i++) if (!pk16_bias_site_ok(site_worst[i])) return false;
    return post_best <= PK16_POST_GAIN_MAX;
}

}  // namespace c4k
