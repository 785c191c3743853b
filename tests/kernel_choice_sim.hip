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
// facts: LaunchFacts' members in the order of kcsim_choose's comment (18 ints)
LaunchFacts facts_from(const int *facts, const int *query_length, int n_lengths) {
    LaunchFacts f;
    f.family = facts[0]; f.mode = facts[1]; f.cont = facts[2]; f.n = facts[3]; f.blocked = facts[4]; f.span = facts[5];
    f.local = facts[6]; f.local_exact = facts[7]; f.starts_pack = facts[8]; f.cont_free = facts[9]; f.seed_mode = facts[10];
    f.kshift = facts[11]; f.fmt16 = facts[12]; f.pk16_params_ok = facts[13]; f.pk16_all_fit = facts[14]; f.tdense_n = facts[15];
    f.ss16_built = facts[16]; f.cu_count = facts[17];
    f.query_length = query_length; f.n_lengths = n_lengths;
    return f;
}
}  // namespace

// facts: family, mode, cont, n, blocked, span, local, local_exact, starts_pack, cont_free, seed_mode, kshift, fmt16,
// pk16_params_ok, pk16_all_fit, tdense_n, ss16_built, cu_count (18 ints); switches: Switches' members in their order (13 ints).
// Returns 0 and the kernel's name, flags = fmt16 | needs_ss16 << 1 | staged_codes << 2; or 1 and the error text in `name`.
extern "C" int kcsim_choose(const int *facts, const int *switches, const int *query_length, int n_lengths, char *name,
                            int name_cap, int *flags) {
    const LaunchFacts f = facts_from(facts, query_length, n_lengths);
    const KernelChoice c = choose_kernel(f, switches_from(switches));
    strncpy(name, c.error ? c.error : c.ki->name, name_cap - 1);
    name[name_cap - 1] = 0;
    *flags = (c.fmt16 ? 1 : 0) | (c.needs_ss16 ? 2 : 0) | (c.staged_codes ? 4 : 0);
    return c.error ? 1 : 0;
}

// The geometry of one kernel of the table, from its KernelInfo: what tests/edge_cases.py derives a form's row boundaries from.
// which 0: the kernel choose_kernel picks for (facts, switches, query_length) as in kcsim_choose; 1: get_kernel_pk16(family,
// Pk16Form index); 2: get_kernel_win16(family, Win16Shape index); 3: get_kernel_ck16(family, Ck16Shape index); 4:
// get_kernel_ck16(family, Ck16RootedShape index).  `family` is read for which != 0 only (0 takes facts[0]).
// geometry = {KernelInfo::R, waves, hbm_carry, pk16_staged_rows(), pk16_staged_rows6()}.  Returns 0 and the kernel's name; or 1
// and the error text (or "not compiled") in `name`, with geometry[0 .. 2] = 0.
extern "C" int kcsim_geometry(int which, int family, int index, const int *facts, const int *switches, const int *query_length,
                              int n_lengths, char *name, int name_cap, int *geometry) {
    const KernelInfo *ki = nullptr;
    const char *error = nullptr;
    if (which == 0) {
        const KernelChoice c = choose_kernel(facts_from(facts, query_length, n_lengths), switches_from(switches));
        if (c.error) error = c.error; else ki = c.ki;
    } else if (which == 1) ki = (index >= 0 && index < PK16_FORMS) ? get_kernel_pk16(family, (Pk16Form)index) : nullptr;
    else if (which == 2) ki = (index >= 0 && index <= WIN16_R4W3N2) ? get_kernel_win16(family, (Win16Shape)index) : nullptr;
    else if (which == 3) ki = (index >= 0 && index <= CK16_R3W2) ? get_kernel_ck16(family, (Ck16Shape)index) : nullptr;
    else if (which == 4) ki = (index >= 0 && index <= CK16R_R4W3N4) ? get_kernel_ck16(family, (Ck16RootedShape)index) : nullptr;
    if (!ki && !error) error = "not compiled";
    strncpy(name, error ? error : ki->name, name_cap - 1);
    name[name_cap - 1] = 0;
    geometry[0] = ki ? ki->R : 0; geometry[1] = ki ? ki->waves : 0; geometry[2] = ki ? ki->hbm_carry : 0;
    geometry[3] = pk16_staged_rows(); geometry[4] = pk16_staged_rows6();
    return error ? 1 : 0;
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
