// c4_hsp_dev.inc — HSP seeding on the device (part of c4_engine.hip: it uses c4gpu_ctx, DevBuf and ResidentSeqs): the kernels
// around c4_hsp_extend.h's extension of one seed, the soft-mask arrays, and the four c4gpu_hsp_extend_* entry points.

using namespace c4hsp;

namespace {

// one lane per seed
template <bool MASKED>
__global__ void hsp_extend_kernel(const HspArgs a, const c4gpu_hsp_seed *__restrict__ seeds, int n_seeds,
                                  const int *__restrict__ submat, c4gpu_hsp *__restrict__ out, int *__restrict__ dropped) {
    __shared__ int sm[24 * 24];
    hsp_load_matrix(sm, submat);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_seeds; k += gridDim.x * blockDim.x) {
        const c4gpu_hsp_seed sd = seeds[k];
        int d = 0;
        out[k] = hsp_seed_extend<MASKED>(hsp_view(a, sm, sd.pair), sd.query_start, sd.target_start, a.seedlen, a.dropoff,
                                         a.threshold, &d);
        if (MASKED) dropped[k] = d;
    }
}

// one lane per horizon chain: its seeds in order, skipped (length -1) while below the running horizon; a dropped seed moves
// the horizon to its masked end, a kept one to the stored HSP's target end (hspset.c:985-995, seed by seed)
template <bool MASKED>
__global__ void hsp_chain_kernel(const HspArgs a, const c4gpu_hsp_seed *__restrict__ seeds, const int *__restrict__ order,
                                 const int *__restrict__ chain_first, int n_chains, const int *__restrict__ horizon0,
                                 const int *__restrict__ submat, c4gpu_hsp *__restrict__ out, int *__restrict__ dropped) {
    __shared__ int sm[24 * 24];
    hsp_load_matrix(sm, submat);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_chains; c += gridDim.x * blockDim.x) {
        int horizon = horizon0[c];
        for (int x = chain_first[c]; x < chain_first[c + 1]; x++) {
            const int k = order[x];
            c4gpu_hsp h{0, 0, -1, 0, 0};
            int d = 0;
            hsp_horizon_step<MASKED>(a, sm, seeds[k], horizon, &h, &d);
            out[k] = h;
            if (MASKED) dropped[k] = d;
        }
    }
}

// ---- soft-masked sequences ---------------------------------------------------------------------------------------------
// Per position of the raw residues, is the strand position starting there masked (match.c:156-158,178-182,212-220)?  A
// symbol is masked when the alphabet's SOFTMASK filter maps it elsewhere than TO_UPPER does (alphabet.h:87,
// alphabet.c:124-129): every lower-case letter but the wildcard itself (`wild`: 'n' for DNA, 'x' for protein).  A strand of
// advance 3 ORs its three bases (Match_3_mask_func: the target of PROTEIN2DNA, both sides of CODON2CODON); the last two
// positions of a sequence start no codon and are never read.  The coded arrays
// fold case away (Submat index), so this reads the raw bytes; built only for a side whose alphabet is soft-masked.
__global__ void softmask_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long n, int advance, int wild) {
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < n; x += (long long)gridDim.x * blockDim.x) {
        int m = 0;
        for (int d = 0; d < advance; d++)
            if (x + d < n) { const int c = in[x + d]; m |= (c >= 'a' && c <= 'z' && c != wild) ? 1 : 0; }
        out[x] = (uint8_t)m;
    }
}

// what an HSPset of `match_type` reads: the coded arrays of a protein2dna batch are exactly what PROTEIN2DNA scoring reads
// (row of the codon at each target position), those of an ungapped:trans batch hold such rows on both sides (CODON2CODON),
// the 1:1 matches use the plain residue rows
bool hsp_match_known(int match_type) { return match_type >= C4GPU_MATCH_DNA2DNA && match_type <= C4GPU_MATCH_CODON2CODON; }
int hsp_family(int match_type) {
    return match_type == C4GPU_MATCH_CODON2CODON ? FAM_UNGAPPED_CODON : match_type == C4GPU_MATCH_PROTEIN2DNA ? FAM_UNGAPPED_P2D : FAM_UNGAPPED;
}
int hsp_query_advance(int match_type) { return match_type == C4GPU_MATCH_CODON2CODON ? 3 : 1; }
int hsp_target_advance(int match_type) { return match_type == C4GPU_MATCH_PROTEIN2DNA || match_type == C4GPU_MATCH_CODON2CODON ? 3 : 1; }
const int32_t *hsp_matrix(const c4gpu_params *params, int match_type) {
    return match_type == C4GPU_MATCH_DNA2DNA ? &params->dna_submat[0][0] : &params->protein_submat[0][0];
}
std::vector<HspJob> hsp_jobs(const ResidentSeqs &seqs, int n_pairs) {
    std::vector<HspJob> jobs(n_pairs);
    for (int i = 0; i < n_pairs; i++) jobs[i] = HspJob{seqs.qoff[i], seqs.toff[i], seqs.qlen[i], seqs.tlen[i]};
    return jobs;
}

// All four entry points: seed by seed (chain == nullptr) or chain by chain; plain (dropped == nullptr) or with the
// two-stage extension of soft-masked sets (hspset.c:981-995), the masks made here for the flagged sides.
int hsp_extend_host(const char *who, c4gpu_ctx *ctx, const c4gpu_params *params, int match_type, const c4gpu_pair *pairs,
                    int32_t n_pairs, int32_t seedlen, int32_t dropoff, int32_t mask_query, int32_t mask_target, int32_t threshold,
                    const c4gpu_hsp_seed *seeds, int32_t n_seeds, const int32_t *chain, int32_t n_chains, const int32_t *horizon0,
                    c4gpu_hsp *out, int32_t *dropped) {
    try {
        if (hipSetDevice(ctx->device) != hipSuccess) return -1;
        if (!hsp_match_known(match_type)) { c4h::set_error("unknown match type"); return -1; }
        if (!n_seeds) return 0;
        const bool masked = dropped != nullptr;
        const int aq = hsp_query_advance(match_type), at = hsp_target_advance(match_type);
        std::vector<int> first, order;
        if (chain) { first.assign((size_t)n_chains + 1, 0); order.resize((size_t)n_seeds); }
        for (int k = 0; k < n_seeds; k++) {
            const c4gpu_hsp_seed &sd = seeds[k];
            if (sd.pair < 0 || sd.pair >= n_pairs || sd.query_start < 0 || sd.target_start < 0 ||
                (chain && (chain[k] < 0 || chain[k] >= n_chains)) ||
                sd.query_start + seedlen * aq > pairs[sd.pair].query_len || sd.target_start + seedlen * at > pairs[sd.pair].target_len) {
                c4h::set_error(chain || masked ? "an HSP seed lies outside its pair or names no chain" : "an HSP seed lies outside its pair");
                return -1;
            }
            if (chain) first[chain[k] + 1]++;
        }
        if (chain) {
            for (int c = 0; c < n_chains; c++) first[c + 1] += first[c];
            std::vector<int> fill(first.begin(), first.end() - 1);
            for (int k = 0; k < n_seeds; k++) order[fill[chain[k]]++] = k;            // index order inside every chain
        }
        ResidentSeqs seqs;
        if (seqs.build(ctx, hsp_family(match_type), params, pairs, n_pairs)) return -1;
        hipStream_t s = ctx->stream;
        // the masks, from the raw residues the batch keeps (the coded arrays have lost the case): the 64 bytes of padding included
        DevBuf<uint8_t> qmask, tmask;
        const long long hq_n = seqs.total_q + 64, ht_n = seqs.total_t + 64;
        if (masked && mask_query) {
            if (qmask.alloc((size_t)hq_n)) return -1;
            hipLaunchKernelGGL(softmask_kernel, dim3(1024), dim3(256), 0, s, seqs.qraw.p, qmask.p, hq_n, aq,
                               match_type == C4GPU_MATCH_DNA2DNA || match_type == C4GPU_MATCH_CODON2CODON ? 'n' : 'x');
        }
        if (masked && mask_target) {
            if (tmask.alloc((size_t)ht_n)) return -1;
            hipLaunchKernelGGL(softmask_kernel, dim3(1024), dim3(256), 0, s, seqs.traw.p, tmask.p, ht_n, at,
                               match_type == C4GPU_MATCH_PROTEIN2PROTEIN ? 'x' : 'n');
        }
        HIP_OK(hipGetLastError());
        const std::vector<HspJob> jobs = hsp_jobs(seqs, n_pairs);
        DevBuf<HspJob> d_jobs;
        DevBuf<c4gpu_hsp_seed> d_seeds;
        DevBuf<c4gpu_hsp> d_out;
        DevBuf<int> d_submat, d_order, d_first, d_h0, d_dropped;
        if (d_jobs.upload(jobs.data(), n_pairs, s) || d_seeds.upload(seeds, n_seeds, s) || d_out.alloc(n_seeds) ||
            (masked && d_dropped.alloc(n_seeds)) || d_submat.upload(hsp_matrix(params, match_type), 24 * 24, s)) return -1;
        if (chain && (d_order.upload(order.data(), n_seeds, s) || d_first.upload(first.data(), (size_t)n_chains + 1, s) ||
                      d_h0.upload(horizon0, n_chains, s))) return -1;
        const HspArgs a{seqs.qcode.p, seqs.tcode.p, qmask.p, tmask.p, d_jobs.p, aq, at, seedlen, dropoff, threshold};
        const int block = 64, grid = std::min(((chain ? n_chains : n_seeds) + block - 1) / block, 65535);
        if (chain)
            hipLaunchKernelGGL(masked ? hsp_chain_kernel<true> : hsp_chain_kernel<false>, dim3(grid), dim3(block), 0, s, a, d_seeds.p,
                               d_order.p, d_first.p, n_chains, d_h0.p, d_submat.p, d_out.p, d_dropped.p);
        else
            hipLaunchKernelGGL(masked ? hsp_extend_kernel<true> : hsp_extend_kernel<false>, dim3(grid), dim3(block), 0, s, a, d_seeds.p,
                               n_seeds, d_submat.p, d_out.p, d_dropped.p);
        HIP_OK(hipGetLastError());
        if (d_out.download(out, n_seeds, s) || (masked && d_dropped.download(dropped, n_seeds, s))) return -1;
        HIP_OK(c4_stream_sync(s));
        return 0;
    } catch (const std::exception &e) {
        c4h::set_error(std::string(who) + ": " + e.what());
        return -1;
    }
}

}  // namespace

extern "C" int c4gpu_hsp_extend_batch(c4gpu_ctx *ctx, const c4gpu_params *params, int match_type, const c4gpu_pair *pairs,
                                      int32_t n_pairs, int32_t seedlen, int32_t dropoff, const c4gpu_hsp_seed *seeds,
                                      int32_t n_seeds, c4gpu_hsp *out) {
    return hsp_extend_host("c4gpu_hsp_extend_batch", ctx, params, match_type, pairs, n_pairs, seedlen, dropoff, 0, 0, 0, seeds, n_seeds,
                           nullptr, 0, nullptr, out, nullptr);
}

extern "C" int c4gpu_hsp_extend_chains(c4gpu_ctx *ctx, const c4gpu_params *params, int match_type, const c4gpu_pair *pairs,
                                       int32_t n_pairs, int32_t seedlen, int32_t dropoff, const c4gpu_hsp_seed *seeds,
                                       int32_t n_seeds, const int32_t *chain, int32_t n_chains, const int32_t *horizon0,
                                       c4gpu_hsp *out) {
    return hsp_extend_host("c4gpu_hsp_extend_chains", ctx, params, match_type, pairs, n_pairs, seedlen, dropoff, 0, 0, 0, seeds, n_seeds,
                           chain, n_chains, horizon0, out, nullptr);
}

extern "C" int c4gpu_hsp_extend_batch_masked(c4gpu_ctx *ctx, const c4gpu_params *params, int match_type, const c4gpu_pair *pairs,
                                             int32_t n_pairs, int32_t seedlen, int32_t dropoff, int32_t mask_query,
                                             int32_t mask_target, int32_t threshold, const c4gpu_hsp_seed *seeds, int32_t n_seeds,
                                             c4gpu_hsp *out, int32_t *dropped) {
    if (!mask_query && !mask_target) {           // nothing is ever masked (Alphabet_is_masked): the plain call, nothing dropped here
        if (n_seeds > 0) memset(dropped, 0, sizeof(int32_t) * (size_t)n_seeds);
        return c4gpu_hsp_extend_batch(ctx, params, match_type, pairs, n_pairs, seedlen, dropoff, seeds, n_seeds, out);
    }
    return hsp_extend_host("c4gpu_hsp_extend_batch_masked", ctx, params, match_type, pairs, n_pairs, seedlen, dropoff, mask_query,
                           mask_target, threshold, seeds, n_seeds, nullptr, 0, nullptr, out, dropped);
}

extern "C" int c4gpu_hsp_extend_chains_masked(c4gpu_ctx *ctx, const c4gpu_params *params, int match_type, const c4gpu_pair *pairs,
                                              int32_t n_pairs, int32_t seedlen, int32_t dropoff, int32_t mask_query,
                                              int32_t mask_target, int32_t threshold, const c4gpu_hsp_seed *seeds, int32_t n_seeds,
                                              const int32_t *chain, int32_t n_chains, const int32_t *horizon0, c4gpu_hsp *out,
                                              int32_t *dropped) {
    if (!mask_query && !mask_target) {
        if (n_seeds > 0) memset(dropped, 0, sizeof(int32_t) * (size_t)n_seeds);
        return c4gpu_hsp_extend_chains(ctx, params, match_type, pairs, n_pairs, seedlen, dropoff, seeds, n_seeds, chain, n_chains,
                                       horizon0, out);
    }
    if (!chain || !horizon0) { c4h::set_error("c4gpu_hsp_extend_chains_masked: no chains given"); return -1; }
    return hsp_extend_host("c4gpu_hsp_extend_chains_masked", ctx, params, match_type, pairs, n_pairs, seedlen, dropoff, mask_query,
                           mask_target, threshold, seeds, n_seeds, chain, n_chains, horizon0, out, dropped);
}
