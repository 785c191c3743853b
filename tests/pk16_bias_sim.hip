// pk16_bias_sim.hip — TEST INFRASTRUCTURE: the guard of the biased packed score pass (exonerate_amd/csrc/c4_pk16_bias.h) and the
// kernel choice with LaunchFacts::pk16_bias_unfit behind C functions, compiled for the host only and linked against libc4gpu.so
// (the real kernel table).  No device call: tests/test_pk16_bias_guard.py walks the guard's edges in the build container.
#include <cstring>

#include "c4_kernel_choice.h"
#include "c4_pk16_bias.h"

using namespace c4k;

// PK16_BIAS, PK16_ADDEND_MAX, PK16_POST_GAIN_MAX, PK16_SCORE_MAX
extern "C" void pkbias_constants(int *out) {
    out[0] = PK16_BIAS; out[1] = PK16_ADDEND_MAX; out[2] = PK16_POST_GAIN_MAX; out[3] = PK16_SCORE_MAX;
}

// one addend (a substitution score, a calc constant, a splice value as the kernel receives it) / one site's worst PSSM sum
extern "C" int pkbias_addend_ok(long long v) { return pk16_bias_addend_ok(v) ? 1 : 0; }
extern "C" int pkbias_site_ok(long long worst_sum) { return pk16_bias_site_ok(worst_sum) ? 1 : 0; }

extern "C" int pkbias_fits(const int *submat, int n_submat, const int *calc_value, int n_calcs, const long long *site_worst,
                           int n_sites, long long post_best) {
    return pk16_bias_fits(submat, n_submat, calc_value, n_calcs, site_worst, n_sites, post_best) ? 1 : 0;
}

// the score pass with dumps of `n` est2genome jobs of query length `qlen` that all fit the packed pass, on 256 compute units, five
// residue codes, every switch at its default; flags as tests/kernel_choice_sim.hip has them
extern "C" int pkbias_choose(int qlen, int n, int bias_unfit, char *name, int name_cap, int *flags) {
    LaunchFacts f;
    f.family = FAM_EST2GENOME; f.mode = MODE_SCORE; f.n = n; f.local = f.local_exact = true; f.seed_mode = 1; f.kshift = 12;
    f.pk16_params_ok = f.pk16_all_fit = true; f.tdense_n = 5; f.cu_count = 256;
    f.query_length = &qlen; f.n_lengths = 1;
    f.pk16_bias_unfit = bias_unfit != 0;
    const KernelChoice c = choose_kernel(f, Switches());
    strncpy(name, c.error ? c.error : c.ki->name, name_cap - 1);
    name[name_cap - 1] = 0;
    *flags = (c.fmt16 ? 1 : 0) | (c.needs_ss16 ? 2 : 0) | (c.staged_codes ? 4 : 0);
    return c.error ? 1 : 0;
}
