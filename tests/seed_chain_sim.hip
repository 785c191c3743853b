// seed_chain_sim.hip — TEST INFRASTRUCTURE: seed_chain_kernel's replay of the horizon entries (exonerate_amd/csrc/c4_seed_dev.inc)
// run on the CPU.
//
// hsp_entry_step is the product's own code (exonerate_amd/csrc/c4_hsp_extend.h), compiled for the host; what is restated here is
// only the loop around it: on the device one lane per run of equal slots in the sorted list, here one plain loop per entry over
// the walk grouped by entry, walk order kept inside an entry.  tests/test_seed_chain_sim.py holds it to replay_opt
// (tests/seed_fused_opt_cases.py) where there is no GPU.  Nothing in the product links this file.
#include <vector>

#include "../exonerate_amd/csrc/c4_hsp_extend.h"

using namespace c4hsp;

// The seeds of a walk over `n_pairs` pairs (coded arrays and masks at jobs[pair].qoff / .toff; a null mask: that side is not
// flagged), seed k on entry[k] (0 .. n_entries - 1; -1: a seed without an entry, a run of its own).  verdict[k]: 0 not extended,
// 1 extended and nothing stored (out[k]: its HSP, for a dropped seed the masked end), 2 kept (out[k]).  Returns the extensions.
extern "C" int seedchainsim_walk(const uint8_t *qcode, const uint8_t *tcode, const uint8_t *qmask, const uint8_t *tmask,
                                 const HspJob *jobs, const int32_t *submat, int aq, int at, int seedlen, int dropoff, int threshold,
                                 int seed_repeat, const c4gpu_hsp_seed *seeds, int n_seeds, const int32_t *entry, int n_entries,
                                 c4gpu_hsp *out, uint8_t *verdict) {
    const HspArgs a{qcode, tcode, qmask, tmask, jobs, aq, at, seedlen, dropoff, threshold};
    const bool masked = qmask || tmask;
    std::vector<std::vector<int>> runs((size_t)n_entries);
    std::vector<int> alone;
    for (int k = 0; k < n_seeds; k++) {
        if (entry[k] < 0) alone.push_back(k);
        else runs[(size_t)entry[k]].push_back(k);
    }
    for (int k : alone) runs.push_back(std::vector<int>{k});
    int n_extended = 0;
    for (const std::vector<int> &run : runs) {
        HspEntry e{0, 0, 0};
        for (int k : run) {
            int dropped = 0;
            c4gpu_hsp h{0, 0, -1, 0, 0};
            const bool ran = masked ? hsp_entry_step<true>(a, submat, seeds[k], seed_repeat, e, &h, &dropped)
                                    : hsp_entry_step<false>(a, submat, seeds[k], seed_repeat, e, &h, nullptr);
            out[k] = h;
            verdict[k] = !ran ? 0 : (!dropped && h.score >= threshold ? 2 : 1);
            n_extended += ran;
        }
    }
    return n_extended;
}
