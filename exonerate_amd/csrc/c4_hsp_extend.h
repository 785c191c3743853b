// c4_hsp_extend.h — the ungapped X-drop extension of one seed, HSPset_seed_hsp (src/comparison/hspset.c:933-997), once.
//
// Depends on nothing of the engine: c4gpu.h types and plain pointers, every routine __host__ __device__ (the LDS loader at
// the end aside), so that tests/hsp_sim.hip holds this very code to the reference's recorded HSPs without a GPU.  The
// kernels of c4_hsp_dev.inc and seed_chain_kernel (c4_seed_dev.inc) are loops around hsp_seed_extend / hsp_horizon_step /
// hsp_entry_step.
// Residues are read through a batch's coded arrays (qcode / tcode = substitution matrix rows; for PROTEIN2DNA tcode holds
// the row of the codon starting at each position).  Seeds of one diagonal neighbourhood read the same cache lines; the work
// per seed is a few hundred bytes, so the kernels are latency- and not bandwidth-bound.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c4gpu.h"

namespace c4hsp {

struct HspJob { long long qoff, toff; int qlen, tlen; };

// what every seed of one launch shares; qmask / tmask: per position, is it soft-masked (null: that side is not)
struct HspArgs {
    const uint8_t *qcode, *tcode, *qmask, *tmask;
    const HspJob *jobs;
    int aq, at, seedlen, dropoff, threshold;         // threshold: the masked form's drop test (the plain one reads none)
};

// one pair as a seed's passes read it
struct HspView {
    const uint8_t *q, *t, *qm, *tm;
    const int *sm;                                   // the 24 x 24 matrix
    int qlen, tlen, aq, at;
    __host__ __device__ __forceinline__ int score(int qp, int tp) const { return sm[q[qp] * 24 + t[tp]]; }
    __host__ __device__ __forceinline__ bool masked(int qp, int tp) const { return (qm && qm[qp]) || (tm && tm[tp]); }
};

__host__ __device__ __forceinline__ HspView hsp_view(const HspArgs &a, const int *sm, int pair) {
    const HspJob jb = a.jobs[pair];
    return HspView{a.qcode + jb.qoff, a.tcode + jb.toff, a.qmask ? a.qmask + jb.qoff : nullptr,
                   a.tmask ? a.tmask + jb.toff : nullptr, sm, jb.qlen, jb.tlen, a.aq, a.at};
}

// HSP_trim_ends (hspset.c:837-870) and HSP_init (:722-741): the seed without its non-positive ends, and what it scores
__host__ __device__ __forceinline__ c4gpu_hsp hsp_trim_init(const HspView &v, int qs, int ts, int length) {
    int i;
    for (i = 0; i < length; i++) {
        if (v.score(qs, ts) > 0) break;
        qs += v.aq; ts += v.at;
    }
    length -= i;
    int qp = qs + length * v.aq - v.aq, tp = ts + length * v.at - v.at;
    while (length > 0) {
        if (v.score(qp, tp) > 0) break;
        length--; qp -= v.aq; tp -= v.at;
    }
    int score = 0;
    for (i = 0, qp = qs, tp = ts; i < length; i++, qp += v.aq, tp += v.at) score += v.score(qp, tp);
    return c4gpu_hsp{qs, ts, length, score, 0};
}

// HSP_extend (:743-812): left, then right, each to its best extension so far, stopping below zero or `dropoff` under the
// best -- and, with `forbid`, in front of the first masked position (:762-765, 794-797)
__host__ __device__ __forceinline__ void hsp_xdrop_round(const HspView &v, c4gpu_hsp &h, int dropoff, bool forbid) {
    const int aq = v.aq, at = v.at;
    int score = h.score, maxscore = h.score, extend, maxext;
    int qp = h.query_start - aq, tp = h.target_start - at;
    for (extend = 1, maxext = 0; qp >= 0 && tp >= 0; extend++) {                                // left
        if (forbid && v.masked(qp, tp)) break;
        score += v.score(qp, tp);
        if (maxscore <= score) { maxscore = score; maxext = extend; }
        else { if (score < 0) break; if (maxscore - score >= dropoff) break; }
        qp -= aq; tp -= at;
    }
    qp = h.query_start + h.length * aq; tp = h.target_start + h.length * at;
    h.query_start -= maxext * aq; h.target_start -= maxext * at; h.length += maxext;
    score = maxscore;
    for (extend = 1, maxext = 0; qp + aq <= v.qlen && tp + at <= v.tlen; extend++) {            // right
        if (forbid && v.masked(qp, tp)) break;
        score += v.score(qp, tp);
        if (maxscore <= score) { maxscore = score; maxext = extend; }
        else { if (score < 0) break; if (maxscore - score >= dropoff) break; }
        qp += aq; tp += at;
    }
    h.length += maxext;
    h.score = maxscore;
}

// HSP_find_cobs (:426-441)
__host__ __device__ __forceinline__ int hsp_cobs(const HspView &v, const c4gpu_hsp &h) {
    int i, score = 0, qp = h.query_start, tp = h.target_start;
    for (i = 0; i < h.length; i++, qp += v.aq, tp += v.at) {
        score += v.score(qp, tp);
        if (score >= (h.score >> 1)) break;
    }
    return i;
}

// One seed past its horizon test.  Plain: trim, initial score, one free round, cobs.  MASKED, the two-stage rule of a
// soft-masked set (:981-995): a forbidding round first; below `threshold` the seed is DROPPED (*dropped = 1, the HSP
// returned is the masked-extended one with cobs 0: the caller forms HSP_target_end from it, :985-989); otherwise the free
// round from the grown ends (its left pass starts from the first stage's score, after that stage has gone right already:
// not one plain extension -- so a MASKED call with both masks null is not the plain one either).
template <bool MASKED>
__host__ __device__ __forceinline__ c4gpu_hsp hsp_seed_extend(const HspView &v, int qs, int ts, int seedlen, int dropoff,
                                                              int threshold, int *dropped) {
    c4gpu_hsp h = hsp_trim_init(v, qs, ts, seedlen);
    if constexpr (MASKED) {
        hsp_xdrop_round(v, h, dropoff, true);
        *dropped = h.score < threshold;
        if (*dropped) return h;
    }
    hsp_xdrop_round(v, h, dropoff, false);
    h.cobs = hsp_cobs(v, h);
    return h;
}

// The horizon rule on one entry (:952-958, :990), seed by seed: false, and nothing else done, for a seed below `horizon`;
// otherwise *h is its HSP and `horizon` that HSP's target end (HSP_target_end: of the masked HSP when dropped, and whether
// HSP_store keeps it or not).
template <bool MASKED>
__host__ __device__ __forceinline__ bool hsp_horizon_step(const HspArgs &a, const int *sm, const c4gpu_hsp_seed sd, int &horizon,
                                                          c4gpu_hsp *h, int *dropped) {
    if (sd.target_start < horizon) return false;
    *h = hsp_seed_extend<MASKED>(hsp_view(a, sm, sd.pair), sd.query_start, sd.target_start, a.seedlen, a.dropoff, a.threshold,
                                 dropped);
    horizon = h->target_start + h->length * a.at;
    return true;
}

// One horizon entry with what --seedrepeat keeps beside it (:950-970): horizon[0], the counter horizon[1] and the diagonal
// tag horizon[2] of one (section, query frame, target frame).  A fresh set's entry is {0, 0, 0}.
struct HspEntry { int horizon, count; unsigned tag; };

// HSPset_seed_hsp on one entry, seed by seed, in the reference's order (:950-995).  With seed_repeat > 1: a seed of another
// diagonal than the entry's tag clears horizon and counter and takes the tag (compared as 32-bit patterns: Sequence.len is a
// guint, so diag_pos + query->len is unsigned); then the horizon test; then only every seed_repeat-th seed that passed it is
// extended (the counter starts over).  false: nothing extended (below the horizon, or held back by the counter).  Otherwise
// *h is the HSP and `horizon` its target end, as for hsp_horizon_step.  With seed_repeat == 1 (REPEAT false: the code is not
// there) counter and tag are never touched and this is hsp_horizon_step on e.horizon.
template <bool MASKED, bool REPEAT>
__host__ __device__ __forceinline__ bool hsp_entry_step_as(const HspArgs &a, const int *sm, const c4gpu_hsp_seed sd, int seed_repeat,
                                                           HspEntry &e, c4gpu_hsp *h, int *dropped) {
    if constexpr (REPEAT) {
        const unsigned tag = (unsigned)sd.target_start * (unsigned)a.aq - (unsigned)sd.query_start * (unsigned)a.at +
                             (unsigned)a.jobs[sd.pair].qlen;
        if (e.tag != tag) { e.horizon = 0; e.count = 0; e.tag = tag; }
        if (sd.target_start < e.horizon) return false;
        if (++e.count < seed_repeat) return false;
        e.count = 0;
    }
    return hsp_horizon_step<MASKED>(a, sm, sd, e.horizon, h, dropped);
}

template <bool MASKED>
__host__ __device__ __forceinline__ bool hsp_entry_step(const HspArgs &a, const int *sm, const c4gpu_hsp_seed sd, int seed_repeat,
                                                        HspEntry &e, c4gpu_hsp *h, int *dropped) {
    return seed_repeat > 1 ? hsp_entry_step_as<MASKED, true>(a, sm, sd, seed_repeat, e, h, dropped)
                           : hsp_entry_step_as<MASKED, false>(a, sm, sd, seed_repeat, e, h, dropped);
}

// the matrix into the block's LDS (device only: every kernel here opens with it)
__device__ __forceinline__ void hsp_load_matrix(int *sm, const int *__restrict__ submat) {
    for (int x = threadIdx.x; x < 24 * 24; x += blockDim.x) sm[x] = submat[x];
    __syncthreads();
}

}  // namespace c4hsp
