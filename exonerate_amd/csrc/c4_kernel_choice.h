// c4_kernel_choice.h — THE place that decides which compiled kernel serves a launch: the forms of the packed passes under
// names, the C4GPU_* switches the decision reads as one snapshot, and the decision itself as pure functions of plain data
// (nothing of the engine, no device call, no switch read on the way): tests/test_kernel_choice.py walks its edges on the host.
#pragma once
#include <algorithm>

#include "c4_config.h"
#include "c4_launch.h"

namespace c4k {

// ---- the forms of the packed 16-bit passes, by name (the numbers are those of the C4GPU_* switches that pick one) -------------
// the packed score pass with column dumps (c4_viterbi16_kernel.h; kernels/kpk16_families.hip holds one row per form)
enum Pk16Form : int {
    PK16_ASM = 0,              // kpk16: every packed instruction its own asm statement; splice values from the int arrays
    PK16_PLAIN = 1,            // kpk16b: vector builtins, the four splice values of a column as one packed entry (ss16); 32-bit dumps
    PK16_COUNTERS = 2,         // kpk16c: kpk16b with progress counters between the cooperating waves instead of barriers
    PK16_DUMP16 = 3,           // kpk16d: kpk16b with 16-bit dump rows (Dump16), what the packed region windows read
    PK16_STAGED_BARRIER = 4,   // kpk16e: kpk16d with its column loop fed from LDS only (staged), a barrier per chunk
    PK16_STAGED = 5,           // kpk16f: the staged form with progress counters: the default
    PK16_STAGED_NW8 = 6,       // kpk16g: kpk16f on eight waves of two rows per lane (at most one pair of jobs per compute unit)
    PK16_STAGED_R6 = 7,        // kpk16h: staged, six rows per lane: queries of 1 024 .. 1 535 rows in one workgroup's strips
    PK16_STAGED_C8 = 8,        // kpk16i: kpk16f with a query profile for eight residue codes (IUPAC-coded targets)
    PK16_STAGED_LONG = 9,      // kpk16j: kpk16h in super-strips of 1 536 rows, one after the other: queries of any length
    PK16_FORMS
};
// the packed region windows (c4_win16_kernel.h): rows per lane (r), waves per SIMD (w), cooperating waves per pair of chains (n)
enum Win16Shape : int {
    WIN16_R4W2 = 0,            // one wave per pair of window chains: the default
    WIN16_R3W3 = 1, WIN16_R2W4 = 2, WIN16_R6W2 = 3,
    WIN16_R4W2N4 = 4,          // the strips of a window on four cooperating waves
    WIN16_R2W4N8 = 5, WIN16_R2W4N4 = 6,
    WIN16_R4W2N2 = 7,          // ... on two
    WIN16_R4W2_AGAIN = 8,      // (no shape of its own: WIN16_R4W2)
    WIN16_R4W3N2 = 9,
};
// the packed checkpoint pass (c4_ckpt16_kernel.h) over every inner state ...
enum Ck16Shape : int { CK16_R4W2 = 0 /* the default */, CK16_R3W2 = 1 };
// ... and rooted: the component of the state the path's END is entered from
enum Ck16RootedShape : int {
    CK16R_R6W2 = 0,            // one wave per pair of jobs, six rows per lane: the default for short queries
    CK16R_R4W2 = 1, CK16R_R3W3 = 2, CK16R_R2W4 = 3,
    CK16R_R4W2N4 = 4,          // the strips on four cooperating waves
    CK16R_R4W2N2 = 5,          // ... on two
    CK16R_R6W2N3 = 6,          // ... six rows per lane on three
    CK16R_R6W2_AGAIN = 7,      // (no shape of its own: CK16R_R6W2)
    CK16R_R4W3N4 = 8,          // four cooperating waves at three waves per SIMD
};

// NULL = not compiled for the family.  The packed score pass is launched over the same job / result arrays as the 32-bit
// kernel (workgroup p runs jobs 2p and 2p + 1); the checkpoint pass and the windows take their pairs from LaunchArgs::aux, and
// scratch.ckpt holds two slabs of ckpt_stride ints per wave.  The rooted checkpoint form is NULL where the family's components overlap.
const KernelInfo *get_kernel_pk16(int family, Pk16Form form);
const KernelInfo *get_kernel_win16(int family, Win16Shape shape);
const KernelInfo *get_kernel_ck16(int family, Ck16Shape shape);
const KernelInfo *get_kernel_ck16(int family, Ck16RootedShape shape);

// ---- the switches the choice reads, as one snapshot -------------------------------------------------------------------------
struct Switches {
    int mw = 1;                // C4GPU_MW: 0: one-wave kernels only; 4: never the eight-wave forms
    int wpe = 0;               // C4GPU_WPE: the waves-per-EU build of the 32-bit kernels (0 for blocked launches whatever it says)
    int pack = 1;              // C4GPU_PACK: 0: region starts in two slots
    int pk16 = 1;              // C4GPU_PK16: 0: no packed score pass; 3: PK16_ASM; 4: PK16_COUNTERS; anything else: PK16_PLAIN,
                               // and 1 EXACTLY: the forms with 16-bit dumps behind it
    int pk16_io = 2;           // C4GPU_PK16_IO: 0: never a staged form; 1: PK16_STAGED_BARRIER and nothing beyond it
    int pk16_c8 = 1;           // C4GPU_PK16_C8: 0: never PK16_STAGED_C8
    int pk16_r6 = 1;           // C4GPU_PK16_R6: 0: never PK16_STAGED_R6 (nor PK16_STAGED_LONG)
    int pk16_long = 1;         // C4GPU_PK16_LONG: 0: never PK16_STAGED_LONG
    int pk16_nw8 = -1;         // C4GPU_PK16_NW8: 0: never PK16_STAGED_NW8; 1: wherever the queries fit; else by the job count
    int win16 = 1;             // C4GPU_WIN16: 0: 32-bit dumps and windows; <= 1: the shape by the jobs; k = 2 .. 10: Win16Shape k - 1,
                               // whatever the jobs (tests, measurement), but 9: WIN16_R4W2
    int win_nw = 2;            // C4GPU_WIN_NW: cooperating waves of the 32-bit windows: 2, anything else means 4
    int ck16 = 1;              // C4GPU_CK16: 0: no packed checkpoint pass; 1: the rooted shape by the jobs; k: Ck16RootedShape k - 1,
                               // but 8: CK16R_R6W2
    int ck16_root = 1;         // C4GPU_CK16_ROOT: 0: never the rooted form
    // read on every call: a test switches them between two calls
    static Switches from_config() {
        Switches s;
        using namespace c4cfg;
        s.mw = num(MW, s.mw); s.wpe = num(WPE, s.wpe); s.pack = num(PACK, s.pack);
        s.pk16 = num(PK16, s.pk16); s.pk16_io = num(PK16_IO, s.pk16_io); s.pk16_c8 = num(PK16_C8, s.pk16_c8);
        s.pk16_r6 = num(PK16_R6, s.pk16_r6); s.pk16_long = num(PK16_LONG, s.pk16_long); s.pk16_nw8 = num(PK16_NW8, s.pk16_nw8);
        s.win16 = num(WIN16, s.win16); s.win_nw = num(WIN_NW, s.win_nw);
        s.ck16 = num(CK16, s.ck16); s.ck16_root = num(CK16_ROOT, s.ck16_root);
        return s;
    }
};

// ---- what the choice looks at -----------------------------------------------------------------------------------------------
struct LaunchFacts {
    int family = 0, mode = 0;
    bool cont = false;
    int n = 0;                         // jobs
    bool blocked = false;              // the launch carries sub-optimal blocking lists
    int span = 0;                      // 0, or BSDP's span seam (get_kernel)
    bool local = false, local_exact = false;       // Engine::local, Engine::local_exact
    bool starts_pack = false;          // every job's (query_start << tshift) | target_start fits 31 bits
    bool cont_free = false;            // the continuation kernels without the row-0 mask stay exact for every job
    int seed_mode = 0;                 // the windowed region pass (SeedPlan): 1: the score pass that dumps, 2: the windows
    int kshift = 0;
    bool fmt16 = false;                // seed_mode 2: the score pass before wrote 16-bit dumps
    bool pk16_params_ok = false;       // Engine::pk16_params_ok
    bool pk16_all_fit = false;         // seed_mode 1: every job passes Engine::pk16_fits
    int tdense_n = 0;                  // residue codes in the batch's targets (0: no dense code table)
    bool ss16_built = false;
    int cu_count = 0;
    const int *query_length = nullptr; // of the jobs of a launch without continuation (the others are not chosen by size)
    int n_lengths = 0;
    bool pk16_bias_unfit = false;      // !Engine::pk16_bias_ok: an addend the biased (staged) forms of the packed score pass cannot carry
};

struct KernelChoice {
    const KernelInfo *ki;
    bool fmt16;                        // what SeedPlan::fmt16 is after this launch
    bool needs_ss16;                   // the kernel reads the packed splice array: build it first
    bool staged_codes;                 // the kernel takes the batch's residue-code table (LaunchArgs::aux)
    const char *error;                 // the launch cannot be served (ki is then meaningless)
};

// cooperating waves per job of the region windows (SEED 2): two where the family has that form -- a job's later windows are
// a few hundred rows high and leave fewer waves idle than with four (north-star batch: 846 against 867 ms per step) --
// three waves: 894-916 ms, one wave with every strip boundary through HBM: 854-872 ms, four rows per lane on two waves:
// 851-857 ms -- C4GPU_WIN_NW=4 keeps four
inline int window_waves(int family, const Switches &sw) {
    const int nw = sw.win_nw == 2 ? 2 : 4;
    return get_kernel_mw(family, MODE_REGION, true, true, nw, false, 2) ? nw : 4;
}

// the form C4GPU_PK16 asks for where the packed score pass serves
inline Pk16Form pk16_base_form(const Switches &sw) { return sw.pk16 == 3 ? PK16_ASM : sw.pk16 == 4 ? PK16_COUNTERS : PK16_PLAIN; }

// "the packed score pass is on for this batch at all": two jobs per lane in packed 16-bit halves (est2genome, parameters far
// inside 16 bits).  Whether it serves a launch is this and Engine::pk16_fits for every job.
inline bool pk16_enabled(int family, bool pk16_params_ok, long long n_jobs, const Switches &sw) {
    return family == FAM_EST2GENOME && pk16_params_ok && n_jobs >= 2 && sw.pk16 != 0 &&
           get_kernel_pk16(family, pk16_base_form(sw)) != nullptr;
}

// the score pass with dumps, where the packed pass serves every job (choose_kernel)
inline void choose_pk16(const LaunchFacts &f, const Switches &sw, KernelChoice &c) {
    c.ki = get_kernel_pk16(f.family, pk16_base_form(sw));
    c.needs_ss16 = sw.pk16 != 3;           // PK16_ASM alone reads the int splice arrays
    // with the packed region windows behind it (c4_win16_kernel.h; C4GPU_WIN16=0: the 32-bit windows) it writes its dumps as
    // 16-bit rows: window rows and columns must fit 15 / 16 bits, and the windows index a query profile by the targets' dense
    // codes: at most eight residue codes in the batch
    if (sw.pk16 != 1 || !sw.win16) return;
    const KernelInfo *kd = get_kernel_pk16(f.family, PK16_DUMP16);
    if (!kd || !get_kernel_win16(f.family, WIN16_R4W2) || f.kshift > 15 || f.tdense_n <= 0) return;
    int rows = 0;                          // of the longest query: Q + 1
    for (int i = 0; i < f.n_lengths; i++) rows = std::max(rows, f.query_length[i] + 1);
    if (rows > 32000) return;
    c.ki = kd; c.fmt16 = true;
    // the staged forms carry their scores biased (c4_viterbi16_kernel.h, BIAS): parameters with an addend that form cannot carry
    // stay on the form that loads per step, with integer maxima
    if (f.pk16_bias_unfit) return;
    // ... and with its column loop fed from LDS alone (staged) where every query fits the strips of one workgroup and the
    // targets hold few enough residue codes for the query profile
    const KernelInfo *ke = sw.pk16_io ? get_kernel_pk16(f.family, sw.pk16_io == 2 ? PK16_STAGED : PK16_STAGED_BARRIER) : nullptr;
    if (!ke) return;
    const bool counters = sw.pk16_io == 2;         // the forms beyond PK16_STAGED exist with progress counters only
    const bool strips_ok = rows <= pk16_staged_rows();
    // seven or eight codes (IUPAC ambiguity codes in the targets): the staged form with the larger profile, where every
    // query fits its four strips of 256 rows
    if (f.tdense_n > pk16_staged_codes() && f.tdense_n <= 8 && counters && sw.pk16_c8 && strips_ok &&
        get_kernel_pk16(f.family, PK16_STAGED_C8)) {
        c.ki = get_kernel_pk16(f.family, PK16_STAGED_C8); c.staged_codes = true;
    }
    if (f.tdense_n > pk16_staged_codes()) return;
    if (strips_ok) {
        c.ki = ke; c.staged_codes = true;
        // ... on eight waves of two rows per lane where the launch has at most one pair of jobs per compute unit (the shard
        // of a strong-scaled run): twice the waves on the same rows
        const KernelInfo *kg = (counters && sw.pk16_nw8 != 0) ? get_kernel_pk16(f.family, PK16_STAGED_NW8) : nullptr;
        if (kg && (sw.pk16_nw8 == 1 || (f.n + 1) / 2 <= f.cu_count)) c.ki = kg;
    } else if (counters && sw.pk16_r6) {
        // queries of 1 024 .. 1 535 rows: six rows per lane put them into the four strips of one workgroup; longer ones in
        // several super-strips of that form; else the form that loads per step, in two passes over the target
        const KernelInfo *kh = get_kernel_pk16(f.family, PK16_STAGED_R6), *kj = get_kernel_pk16(f.family, PK16_STAGED_LONG);
        if (kh && rows <= pk16_staged_rows6()) { c.ki = kh; c.staged_codes = true; }
        else if (kj && sw.pk16_long) { c.ki = kj; c.staged_codes = true; }
    }
}

// Which kernel serves the launch `f` describes.  Launches nothing, changes nothing.
inline KernelChoice choose_kernel(const LaunchFacts &f, const Switches &sw) {
    KernelChoice c{nullptr, f.fmt16, false, false, nullptr};
    const bool rect = !f.cont && (f.mode == MODE_SCORE || f.mode == MODE_REGION);       // a whole-rectangle pass
    const bool use_local = f.local && f.local_exact && rect;
    // packed region-start slot; C4GPU_PACK=0 forces the two-slot form (what targets beyond 2^31 / query-rows columns get)
    const bool pack = f.mode == MODE_REGION && sw.pack && f.starts_pack;
    const int wpe = f.blocked ? 0 : sw.wpe;
    c.ki = get_kernel(f.family, f.mode, f.cont, f.cont ? f.cont_free : use_local, pack, wpe, f.blocked, f.span);
    if (!c.ki && f.cont_free) c.ki = get_kernel(f.family, f.mode, f.cont, false, pack, wpe, f.blocked, f.span);
    if (!c.ki) { c.error = "no compiled kernel for this model/mode"; return c; }
    auto strips_of = [&](int rows_per_strip) {
        long long strips = 0;
        for (int i = 0; i < f.n_lengths; i++) strips += (f.query_length[i] + 1 + rows_per_strip - 1) / rows_per_strip;
        return strips;
    };
    // too few jobs to occupy the device on four waves each: eight waves of half the rows (C4GPU_MW=4 keeps four)
    const bool few_jobs = (long long)f.n * 8 <= 2LL * 4 * f.cu_count;
    if (f.seed_mode) {
        int nw = f.seed_mode == 2 ? window_waves(f.family, sw) : 4;
        // (256 proteins against one chromosome)
        if (f.seed_mode == 1 && sw.mw != 4 && few_jobs && get_kernel_mw(f.family, f.mode, true, false, 8, false, 1)) nw = 8;
        c.ki = get_kernel_mw(f.family, f.mode, true, f.mode == MODE_REGION, nw, false, f.seed_mode);
        if (!c.ki || !use_local || (f.mode == MODE_REGION && !pack)) { c.error = "no seeded kernel for this launch"; return c; }
        if (f.seed_mode == 1 && pk16_enabled(f.family, f.pk16_params_ok, f.n, sw) && f.pk16_all_fit) choose_pk16(f, sw, c);
        if (f.seed_mode == 2 && f.fmt16) {
            int shape = sw.win16 == 9 ? WIN16_R4W2 : sw.win16 - 1;
            if (sw.win16 <= 1) {
                // the strips of a window on two cooperating waves where the first windows have two strips and more, on four
                // where the launch has at most one pair of jobs per compute unit (the shard of a strong-scaled run: 512 pairs,
                // region windows 30.5 -> 20.7 ms per step, profiles/r05_shard_sweep.log)
                shape = strips_of(256) < 2LL * f.n ? WIN16_R4W2 : (f.n + 1) / 2 <= f.cu_count ? WIN16_R4W2N4 : WIN16_R4W2N2;
            }
            c.ki = get_kernel_win16(f.family, (Win16Shape)shape);
            if (!c.ki || !f.ss16_built) { c.error = "no packed window kernel for this launch"; return c; }
        }
    } else if (sw.mw && rect) {
        // whole-rectangle passes whose query spans several 64*R-row strips run on 4 cooperating waves per job (strip carry
        // rows stay in LDS instead of HBM); C4GPU_MW=0 forces the one-wave kernels
        const KernelInfo *kmw = get_kernel_mw(f.family, f.mode, use_local, pack, 4, f.blocked);
        if (kmw && strips_of(64 * kmw->R) >= 3LL * f.n) {
            c.ki = kmw;
            // 8 waves x 2 rows per lane cover the same rows per workgroup with twice the waves
            const KernelInfo *kmw8 = (sw.mw != 4 && !f.blocked) ? get_kernel_mw(f.family, f.mode, use_local, pack, 8) : nullptr;
            if (kmw8 && few_jobs) c.ki = kmw8;
        }
    }
    return c;
}

// The rooted packed checkpoint pass, by the strips of 256 rows its jobs have: four (two) cooperating waves per pair of jobs
// where the jobs fill them -- the launch then lasts as long as its work, not as its longest job's strips one after the other
// (north-star batch, two lanes: 481 -> 446 ms per step; profiles/r04_ck16_sweep.log) --, one wave per pair of short queries;
// the four-wave shape at three waves per SIMD, 168 registers: 65 -> 52 ms per launch, step 436 -> 430 ms
// (profiles/r04_ck16_w3_sweep.log).  C4GPU_CK16 = 2 .. : one shape whatever the jobs.
inline Ck16RootedShape choose_ck16_rooted_shape(int family, long long strips, int n_rooted, int rows_max, const Switches &sw) {
    if (sw.ck16 != 1) return sw.ck16 == 8 ? CK16R_R6W2 : (Ck16RootedShape)(sw.ck16 - 1);
    // regions of 1 025 .. 1 152 rows are five strips of 256 -- a second round for one wave of four -- and three strips of
    // 384: the six-rows-per-lane shape on three waves takes them in one round (cDNAs of 1.1 kb)
    if (rows_max > 1024 && rows_max <= 3 * 384 && strips >= 4LL * n_rooted && get_kernel_ck16(family, CK16R_R6W2N3))
        return CK16R_R6W2N3;
    return strips >= 3LL * n_rooted ? CK16R_R4W3N4 : strips >= 2LL * n_rooted ? CK16R_R4W2N2 : CK16R_R6W2;
}

}  // namespace c4k
