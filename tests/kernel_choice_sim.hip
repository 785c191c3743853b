// kernel_choice_sim.hip — TEST INFRASTRUCTURE: the product's kernel choice (exonerate_amd/csrc/c4_kernel_choice.h) behind a C
// function, compiled for the host only and linked against libc4gpu.so, so that it looks the kernels up in the real table.
// No device call: tests/test_kernel_choice.py walks the edges of the choice in the build container.
#include <climits>
#include <cstring>

#include "c4_kernel_choice.h"

using namespace c4k;

namespace {
// switches[k] == INT_MIN: the default the product has
Switches switches_from(const int *v) {
    Switches s;
    int *const field[13] = {&s.mw, &s.wpe, &s.pack, &s.pk16, &s.pk16_io, &s.pk16_c8, &s.pk16_r6, &s.pk16_long, &s.pk16_nw8,
                            &s.win16, &s.win_nw, &s.ck16, &s.ck16_root};
    for (int k = 0; k < 13; k++) if (v[k] != INT_MIN) *field[k] = v[k];
    return s;
}
}  // namespace

// facts: family, mode, cont, n, blocked, span, local, local_exact, starts_pack, cont_free, seed_mode, kshift, fmt16,
// pk16_params_ok, pk16_all_fit, tdense_n, ss16_built, cu_count (18 ints); switches: Switches' members in their order (13 ints).
// Returns 0 and the kernel's name, flags = fmt16 | needs_ss16 << 1 | staged_codes << 2; or 1 and the error text in `name`.
extern "C" int kcsim_choose(const int *facts, const int *switches, const int *query_length, int n_lengths, char *name,
                            int name_cap, int *flags) {
    LaunchFacts f;
    f.family = facts[0]; f.mode = facts[1]; f.cont = facts[2]; f.n = facts[3]; f.blocked = facts[4]; f.span = facts[5];
    f.local = facts[6]; f.local_exact = facts[7]; f.starts_pack = facts[8]; f.cont_free = facts[9]; f.seed_mode = facts[10];
    f.kshift = facts[11]; f.fmt16 = facts[12]; f.pk16_params_ok = facts[13]; f.pk16_all_fit = facts[14]; f.tdense_n = facts[15];
    f.ss16_built = facts[16]; f.cu_count = facts[17];
    f.query_length = query_length; f.n_lengths = n_lengths;
    const KernelChoice c = choose_kernel(f, switches_from(switches));
    strncpy(name, c.error ? c.error : c.ki->name, name_cap - 1);
    name[name_cap - 1] = 0;
    *flags = (c.fmt16 ? 1 : 0) | (c.needs_ss16 ? 2 : 0) | (c.staged_codes ? 4 : 0);
    return c.error ? 1 : 0;
}

// the rooted packed checkpoint kernel for `n_rooted` est2genome jobs with `strips` strips of 256 rows, the longest of `rows_max` rows
extern "C" void kcsim_ck16_rooted(long long strips, int n_rooted, int rows_max, const int *switches, char *name, int name_cap) {
    const KernelInfo *ki = get_kernel_ck16(FAM_EST2GENOME, choose_ck16_rooted_shape(FAM_EST2GENOME, strips, n_rooted, rows_max,
                                                                                    switches_from(switches)));
    strncpy(name, ki->name, name_cap - 1);
    name[name_cap - 1] = 0;
}

// pk16_enabled, as the stage and find_path_batch ask it
extern "C" int kcsim_pk16_enabled(int family, int params_ok, int n_jobs, const int *switches) {
    return pk16_enabled(family, params_ok != 0, n_jobs, switches_from(switches)) ? 1 : 0;
}
