// the packed 16-bit score pass (c4_viterbi16_kernel.h): two jobs per lane, 4 rows per lane, 4 waves per pair of jobs, held to
// 3 waves per SIMD — the best of the shapes measured (profiles/r03_pk16.md).  est2genome only: for protein2dna (no shadow
// payload to shed, a ring of four columns) the packed pass is 38 % SLOWER than the 32-bit one on config 3's shape
// (2 356 against 1 706 ms per pass), and affine runs no whole-rectangle score pass at config 2's size.
#include "../c4_kernel_choice.h"
#include "../c4_viterbi16_kernel.h"
namespace c4k {
// one form of the pass: the launcher, the occupancy handle and the sizes the host lays its buffers out by all follow from ONE
// template argument list (IO 1, the staged forms: the launch's residue-code table arrives in LaunchArgs::aux)
// (every staged form carries its scores biased, BIAS: the match states' maxima two candidates per instruction)
template <class M, int R, int NW, int WPE, int VAR, bool D16, int IO = 0, int NCODE = 6, bool MEMC = false>
struct Pk16 {
    using DP = WaveDP16<M, R, VAR, D16, IO, NCODE, MEMC, IO == 1>;
    static constexpr auto kernel = viterbi16_kernel_mw<M, R, NW, WPE, VAR, D16, IO, NCODE, MEMC, IO == 1>;
    static hipError_t launch(const LaunchArgs &a) {
        hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(64 * NW), 0, a.stream, a.kp, a.seqs, a.jobs, a.n_jobs, a.results, a.scratch,
                           a.queue, IO ? reinterpret_cast<const uint8_t *>(a.aux) : nullptr);
        return hipGetLastError();
    }
    static KernelInfo info(const char *name) {
        return {launch, (const void *)kernel, name, R, 2, DP::BND, M::NS, M::MAXAT, NW, DP::SEEDW};
    }
};
// indexed by Pk16Form (c4_kernel_choice.h says what each form is for).  What the shapes cost and gained:
// kpk16f: a wave starts chunk k once the wave above has finished chunk k + 2 and the wave below chunk k - 5 (the ring slots it
//   overwrites have been read): 303 -> 297 ms per launch of 4 096 pairs now that the four waves do the same work
// kpk16g: 256 pairs of jobs on 256 CUs would otherwise be one wave per SIMD, which issues an instruction every ~5 cycles whatever
//   else is free
// kpk16h: strips of 384 rows, two waves per SIMD; four rows per lane need a second pass over the target for rows 1 024 ..: cDNAs of
//   1.1 kb ran at half the rate of 1 kb ones (bench.py configs.c4_query_1100)
// kpk16i: the six-code form sent IUPAC-coded batches to the form that loads per step, 0.77 of the rate (bench.py
//   configs.c4_eight_codes): 61.6 KB of LDS, two workgroups per CU, two waves per SIMD (256 registers: nothing in scratch)
// kpk16j: the row between two super-strips goes through the workgroup's slab in memory (MEMC): cDNAs of 1.6 - 3 kb (up to ~3 190
//   rows, what the packed guard lets through) stay on the staged form, in two or three passes over the target
using E = Est2GenomeDesc;
static const KernelInfo pk16_forms[PK16_FORMS] = {
    //   R NW WPE VAR D16   IO NCODE MEMC
    Pk16<E, 4, 4, 3, 0, false>::info("kpk16_est2genome"),
    Pk16<E, 4, 4, 3, 1, false>::info("kpk16b_est2genome"),
    Pk16<E, 4, 4, 3, 2, false>::info("kpk16c_est2genome"),
    Pk16<E, 4, 4, 3, 1, true>::info("kpk16d_est2genome"),
    Pk16<E, 4, 4, 3, 1, true, 1>::info("kpk16e_est2genome"),
    Pk16<E, 4, 4, 3, 2, true, 1>::info("kpk16f_est2genome"),
    Pk16<E, 2, 8, 2, 2, true, 1>::info("kpk16g_est2genome"),
    Pk16<E, 6, 4, 2, 2, true, 1>::info("kpk16h_est2genome"),
    Pk16<E, 4, 4, 2, 2, true, 1, 8>::info("kpk16i_est2genome"),
    Pk16<E, 6, 4, 2, 2, true, 1, 6, true>::info("kpk16j_est2genome"),
};
static int rows_of(Pk16Form f) { return pk16_forms[f].R * 64 * pk16_forms[f].waves; }
int pk16_staged_codes() { return Pk16<E, 4, 4, 3, 2, true, 1>::DP::NCODE; }
int pk16_staged_rows() { return rows_of(PK16_STAGED); }
int pk16_staged_rows6() { return rows_of(PK16_STAGED_R6); }
// the packed splice array of variant 1 (ss16_kernel): n positions of the batch's concatenated targets
hipError_t pk16_build_splice(int family, const KParams *kp, const int *ss, long long ss_stride, long long n, void *out, hipStream_t s) {
    if (family != FAM_EST2GENOME) return hipErrorInvalidValue;
    hipLaunchKernelGGL((ss16_kernel<Est2GenomeDesc>), dim3(4096), dim3(256), 0, s, kp, ss, ss_stride, n, (uint2 *)out);
    return hipGetLastError();
}
const KernelInfo *get_kernel_pk16(int family, Pk16Form form) {
    if (family != FAM_EST2GENOME) return nullptr;
    return &pk16_forms[form >= 0 && form < PK16_FORMS ? form : PK16_ASM];
}
}
