// hsp_sim.hip — TEST INFRASTRUCTURE: the HSP extension of one seed (exonerate_amd/csrc/c4_hsp_extend.h) run on the CPU.
//
// hsp_seed_extend and hsp_horizon_step are the product's own code, compiled for the host; what is restated here is only the
// loop around them (one lane per seed / per horizon chain on the device, one plain loop here).  tests/test_hsp_sim.py holds
// it to the reference's recorded HSPs and to the Python restatement of tests/test_hsp_softmask.py where there is no GPU.
// Nothing in the product links this file.
#include "../exonerate_amd/csrc/c4_hsp_extend.h"

using namespace c4hsp;

namespace {
// one pair at offset 0 of its coded (and mask) arrays
struct OnePair {
    HspJob job;
    HspArgs a;
    OnePair(const uint8_t *qcode, const uint8_t *tcode, const uint8_t *qmask, const uint8_t *tmask, int qlen, int tlen, int aq, int at,
            int seedlen, int dropoff, int threshold)
        : job{0, 0, qlen, tlen}, a{qcode, tcode, qmask, tmask, &job, aq, at, seedlen, dropoff, threshold} {}
};
}  // namespace

// One seed, plain (masked == 0: the masks and the threshold are not read) or with the two-stage rule: its HSP, whether dropped.
extern "C" int hspsim_seed(int masked, const uint8_t *qcode, const uint8_t *tcode, const uint8_t *qmask, const uint8_t *tmask,
                           int qlen, int tlen, const int32_t *submat, int aq, int at, int seedlen, int dropoff, int threshold,
                           int query_start, int target_start, c4gpu_hsp *out) {
    const OnePair p(qcode, tcode, qmask, tmask, qlen, tlen, aq, at, seedlen, dropoff, threshold);
    const HspView v = hsp_view(p.a, submat, 0);
    int dropped = 0;
    *out = masked ? hsp_seed_extend<true>(v, query_start, target_start, seedlen, dropoff, threshold, &dropped)
                  : hsp_seed_extend<false>(v, query_start, target_start, seedlen, dropoff, threshold, nullptr);
    return dropped;
}

// The seeds of one pair in order, seed k on horizon entry chain[k] (every entry starts at 0): out[k].length == -1 and
// dropped[k] == 0 for a skipped seed, as the chain kernels report it.
extern "C" void hspsim_walk(int masked, const uint8_t *qcode, const uint8_t *tcode, const uint8_t *qmask, const uint8_t *tmask,
                            int qlen, int tlen, const int32_t *submat, int aq, int at, int seedlen, int dropoff, int threshold,
                            const c4gpu_hsp_seed *seeds, int n_seeds, const int32_t *chain, int32_t *horizon, c4gpu_hsp *out,
                            int32_t *dropped) {
    const OnePair p(qcode, tcode, qmask, tmask, qlen, tlen, aq, at, seedlen, dropoff, threshold);
    for (int k = 0; k < n_seeds; k++) {
        out[k] = c4gpu_hsp{0, 0, -1, 0, 0};
        int d = 0;
        if (masked) hsp_horizon_step<true>(p.a, submat, seeds[k], horizon[chain[k]], &out[k], &d);
        else hsp_horizon_step<false>(p.a, submat, seeds[k], horizon[chain[k]], &out[k], nullptr);
        dropped[k] = d;
    }
}
