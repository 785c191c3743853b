// c4_sdp_dev.inc — c4gpu_sdp_batch: SDP (seeded dynamic programming, src/sdp/) for every pair of a batch on the device.
// Part of c4_engine.hip (it uses c4gpu_ctx, DevBuf and ResidentSeqs).  The passes are the sparse wavefront kernels of
// c4_sdp_wave.h (one wave per pair, both flavours of SDP_create sdp.c:322-366), the host side is c4_sdp_host.h.
//
// Memory: the passes append step records to per-pair streams that grow in 64 KB chunks out of ONE arena kept in the
// context (grown, never shrunk): proportional to the steps the X-drop visits, whatever the lattice sizes.  A pair whose
// streams do not fit (arena exhausted) is run once more with an arena eight times the size and, failing that, reported
// as not served (n_out[i] = -1): it never takes the other pairs of the batch down with it.

namespace {
using namespace c4sdp;

const SdpFamilyInfo *sdp_family_info(int family, const SdpKernels **k) {
    switch (family) {
        case FAM_AFFINE: { static const SdpFamilyInfo f = make_family_info<AffineDesc, false>(); *k = sdp_kernels_affine(); return &f; }
        case FAM_PROTEIN2DNA: { static const SdpFamilyInfo f = make_family_info<Protein2DnaDesc, false>(); *k = sdp_kernels_protein2dna(); return &f; }
        case FAM_EST2GENOME: { static const SdpFamilyInfo f = make_family_info<Est2GenomeDesc, true>(); *k = sdp_kernels_est2genome(); return &f; }
        case FAM_PROTEIN2GENOME: { static const SdpFamilyInfo f = make_family_info<Protein2GenomeDesc, true>(); *k = sdp_kernels_protein2genome(); return &f; }
        case FAM_CODING2CODING: { static const SdpFamilyInfo f = make_family_info<Coding2CodingDesc, false>(); *k = sdp_kernels_coding2coding(); return &f; }
        case FAM_CODING2GENOME: { static const SdpFamilyInfo f = make_family_info<Coding2GenomeDesc, true>(); *k = sdp_kernels_coding2genome(); return &f; }
        default: return nullptr;                   // ungapped:trans has no SDP in the reference; ner's spans run along the query
    }
}

// the passes and the walks of one plan; out.status[job] says which jobs were served
int sdp_run_device(c4gpu_ctx *ctx, const SdpFamilyInfo &fi, const SdpKernels &kern, const ResidentSeqs &seqs, const KParams *d_kp,
                   const SdpHostPlan &plan, unsigned arena_chunks, int dropoff, c4gpu_score threshold, SdpBackendOut &out,
                   double *ms_pass, double *ms_walk, unsigned *chunks_used) {
    hipStream_t s = ctx->stream;
    const int n_jobs = (int)plan.jobs.size(), n_seeds = (int)plan.seed_job.size();
    const size_t arena_bytes = (size_t)arena_chunks << CHUNK_LOG;
    if (ctx->sdp_arena_bytes < arena_bytes) {
        const auto ta = std::chrono::steady_clock::now();
        if (ctx->sdp_arena) (void)hipFree(ctx->sdp_arena);
        ctx->sdp_arena = nullptr; ctx->sdp_arena_bytes = 0;
        HIP_OK(dev_malloc(&ctx->sdp_arena, arena_bytes));
        ctx->sdp_arena_bytes = arena_bytes;
        if (c4cfg::has(c4cfg::TRACE))
            fprintf(stderr, "c4gpu trace: sdp arena of %.1f GB allocated in %.1f ms\n", arena_bytes / 1e9,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count());
    }
    DevBuf<SdpJob> d_jobs; DevBuf<SdpDSeed> d_rseeds, d_fseeds; DevBuf<int> d_seed_job, d_tabs, d_dirs, d_status;
    DevBuf<SdpBest> d_brev, d_bfwd; DevBuf<unsigned> d_next, d_runs; DevBuf<unsigned long long> d_used; DevBuf<SdpWalkOut> d_orev, d_ofwd;
    std::vector<int> zeros(n_jobs, 0);
    const unsigned zero_u = 0;
    const unsigned long long zero_ull = 0;
    const unsigned long long runs_cap = std::min<unsigned long long>(64ull << 20, std::max<unsigned long long>(1ull << 20, 512ull * n_seeds));
    if (d_jobs.upload(plan.jobs.data(), n_jobs, s) || d_rseeds.upload(plan.rev_seeds.data(), n_seeds, s) ||
        d_fseeds.upload(plan.fwd_seeds.data(), n_seeds, s) || d_seed_job.upload(plan.seed_job.data(), n_seeds, s) ||
        d_tabs.alloc(plan.tabs_total) || d_dirs.alloc(plan.dirs_total) || d_status.upload(zeros.data(), n_jobs, s) ||
        d_brev.alloc(n_seeds) || d_bfwd.alloc(n_seeds) || d_next.upload(&zero_u, 1, s) || d_used.upload(&zero_ull, 1, s) ||
        d_runs.alloc(2 * runs_cap) || d_orev.alloc(n_seeds) || d_ofwd.alloc(n_seeds)) return -1;
    SdpLaunch A;
    memset(&A, 0, sizeof A);
    A.kp = d_kp; A.jobs = d_jobs.p; A.qcode = seqs.dev.qcode; A.tcode = seqs.dev.tcode; A.ss = seqs.dev.ss; A.ss_stride = seqs.dev.ss_stride;
    A.tn4 = seqs.dev.tn4; A.arena = (uint8_t *)ctx->sdp_arena; A.arena_next = d_next.p; A.n_chunks = arena_chunks;
    A.tabs = d_tabs.p; A.dirs = d_dirs.p; A.best_rev = d_brev.p; A.best_fwd = d_bfwd.p; A.status = d_status.p; A.dropoff = dropoff;
    HIP_OK(hipEventRecord(ctx->ev0, s));
    A.seeds = d_rseeds.p;
    HIP_OK(kern.rev(A, n_jobs, s));
    A.seeds = d_fseeds.p;
    HIP_OK(kern.fwd(A, n_jobs, s));
    HIP_OK(hipEventRecord(ctx->ev1, s));
    // (destroyed on every way out of this function; c4gpu_sdp_batch is called from one thread per context: the arena and the
    // context's events are not shared between callers)
    struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } ev2g;
    HIP_OK(hipEventCreate(&ev2g.e));
    hipEvent_t ev2 = ev2g.e;
    SdpWalkLaunch W;
    memset(&W, 0, sizeof W);
    W.jobs = d_jobs.p; W.seed_job = d_seed_job.p; W.gate = d_bfwd.p; W.arena = (const uint8_t *)ctx->sdp_arena; W.tabs = d_tabs.p;
    W.dirs = d_dirs.p; W.status = d_status.p; W.n_seeds = n_seeds; W.threshold = threshold; W.runs = d_runs.p; W.runs_used = d_used.p;
    W.runs_cap = runs_cap;
    W.tab = fi.walk_fwd; W.best = d_bfwd.p; W.out = d_ofwd.p;
    hipLaunchKernelGGL(sdp_walk_kernel2, dim3((n_seeds + 63) / 64), dim3(64), 0, s, W);
    HIP_OK(hipGetLastError());
    if (!fi.bnd) {
        W.tab = fi.walk_rev; W.best = d_brev.p; W.out = d_orev.p;
        hipLaunchKernelGGL(sdp_walk_kernel2, dim3((n_seeds + 63) / 64), dim3(64), 0, s, W);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(ev2, s));
    out.status.assign(n_jobs, 0);
    out.fwd.assign(n_seeds, SdpWalkOut{}); out.rev.assign(n_seeds, SdpWalkOut{});
    unsigned long long used = 0;
    unsigned next_chunk = 0;
    // The read-backs are queued only once the passes are over.  A DMA copy queued behind a kernel waits in its engine's queue
    // for that kernel, and the engines' queues are shared by every stream of the process: the uploads of ANOTHER thread (the
    // drop-in's main thread scanning the next target beside this batch, integration/c4gpu_sdp.c) then sat behind these
    // read-backs for the whole 0.36 s of the passes (C4GPU_TRACE laps of c4gpu_seed_scan; tools/two_streams_microbench.hip
    // shows a long kernel alone holds nothing up).
    HIP_OK(c4_stream_sync(s));
    if (d_next.download(&next_chunk, 1, s) || d_status.download(out.status.data(), n_jobs, s) || d_ofwd.download(out.fwd.data(), n_seeds, s) ||
        (!fi.bnd && d_orev.download(out.rev.data(), n_seeds, s)) || d_used.download(&used, 1, s)) return -1;
    HIP_OK(c4_stream_sync(s));
    used = std::min(used, runs_cap);
    out.runs.resize(2 * used);
    if (used) { if (d_runs.download(out.runs.data(), 2 * used, s)) return -1; HIP_OK(c4_stream_sync(s)); }
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, ctx->ev0, ctx->ev1);
    (void)hipEventElapsedTime(&b, ctx->ev1, ev2);
    if (ms_pass) *ms_pass += a;
    if (ms_walk) *ms_walk += b;
    if (chunks_used) *chunks_used = next_chunk;
    return 0;
}

// how many arena chunks the plan's streams are expected to take.  Measured (profiles/r03_sdp_kernels.md): 21 916 chunks for
// 1 280 seeds / 52 380 HSP positions on the north-star-shaped est2genome run, 327 826 for 33 912 seeds / 372 729 positions on
// config 5's protein2genome pairs: both are 6.9 per seed + 0.25 per position.  The guess is 1.3 x that + 8 per job.  A pair
// that does not fit is run again with eight times the arena (c4gpu_sdp_batch), so a low guess costs one more pass of those
// pairs, a high one an allocation that takes longer than the passes (~14 ms per GB).
unsigned sdp_arena_guess(const std::vector<std::vector<SdpHostSeed>> &seeds, const SdpHostPlan &plan) {
    double n_seeds = 0, positions = 0;
    for (size_t jx = 0; jx < plan.jobs.size(); jx++)
        for (const SdpHostSeed &h : seeds[plan.job_pair[jx]]) { n_seeds += 1; positions += h.hsp->length; }
    const double chunks = 1.3 * (7.0 * n_seeds + 0.25 * positions) + 8.0 * plan.jobs.size() + 256.0;
    return (unsigned)std::min(chunks, 4.0e6);
}

}  // namespace

// the cells of the box around a pair's HSPs (widened by 384 positions): an upper bound of what the passes of
// c4gpu_sdp_batch can visit when nothing extends past the margin; kept for callers that plan by size
extern "C" double c4gpu_sdp_lattice_cells(const c4gpu_hsp *hsps, int32_t n_hsps, int32_t query_advance, int32_t target_advance,
                                          int32_t query_len, int32_t target_len) {
    if (n_hsps <= 0) return ((double)query_len + 1.0) * ((double)target_len + 1.0);
    int qlo = query_len, qhi = 0, tlo = target_len, thi = 0;
    for (int k = 0; k < n_hsps; k++) {
        qlo = std::min(qlo, hsps[k].query_start); qhi = std::max(qhi, hsps[k].query_start + hsps[k].length * query_advance);
        tlo = std::min(tlo, hsps[k].target_start); thi = std::max(thi, hsps[k].target_start + hsps[k].length * target_advance);
    }
    const int margin = 384;
    const double q = std::min(query_len, qhi + margin) - std::max(0, qlo - margin), t = std::min(target_len, thi + margin) - std::max(0, tlo - margin);
    return (q + 1.0) * (t + 1.0);
}

static thread_local struct { double pass_ms, walk_ms, host_ms, stage_ms; long long pairs, jobs, reruns, unserved; } g_sdp_stats;

// statistics of the calling thread's c4gpu_sdp_batch calls since the last reset: kernel time of the passes and of the
// walks (HIP events), staging and host time, jobs launched, pairs run again with a larger arena, pairs not served
extern "C" void c4gpu_sdp_stats(int reset, double *pass_ms, double *walk_ms, double *stage_ms, double *host_ms, int64_t *jobs,
                                int64_t *reruns, int64_t *unserved) {
    if (pass_ms) *pass_ms = g_sdp_stats.pass_ms;
    if (walk_ms) *walk_ms = g_sdp_stats.walk_ms;
    if (stage_ms) *stage_ms = g_sdp_stats.stage_ms;
    if (host_ms) *host_ms = g_sdp_stats.host_ms;
    if (jobs) *jobs = g_sdp_stats.jobs;
    if (reruns) *reruns = g_sdp_stats.reruns;
    if (unserved) *unserved = g_sdp_stats.unserved;
    if (reset) memset(&g_sdp_stats, 0, sizeof g_sdp_stats);
}

// The loop of GAM_Result_SDP_create (gam.c:852-890) for every pair of a batch: SDP_Pair_create_seed_list (sdp.c:438-477),
// the reverse pass and the forward pass of every pair (SDP_Pair_find_start_points / _find_end_points, sdp.c:538-600) in
// two launches, the walks, then SDP_Pair_next_path's single-pass loop (sdp.c:743-815) on the host.
extern "C" int c4gpu_sdp_batch(c4gpu_ctx *ctx, const c4gpu_model *model, const c4gpu_params *params, const c4gpu_pair *pairs,
                               int32_t n_pairs, const c4gpu_hsp *hsps, const int32_t *hsp_first, int32_t query_advance,
                               int32_t target_advance, int32_t dropoff, c4gpu_score threshold, int32_t max_alignments,
                               c4gpu_alignment *out, int32_t *n_out) {
  try {
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return -1; }
    const int family = model_family(*model);
    const SdpKernels *kern = nullptr;
    const SdpFamilyInfo *fi = family >= 0 ? sdp_family_info(family, &kern) : nullptr;
    if (!fi) { c4h::set_error("SDP: this model has no device passes"); return -1; }
    const bool verbose = c4cfg::has(c4cfg::TRACE);
    const auto t0 = std::chrono::steady_clock::now();
    // the seed list of every pair; only pairs with seeds are staged (sequences shared by pointer are staged once)
    std::vector<std::vector<SdpHostSeed>> seeds(n_pairs);
    std::vector<int> staged;
    for (int i = 0; i < n_pairs; i++) {
        n_out[i] = 0;
        sdp_seed_list(hsps + hsp_first[i], hsp_first[i + 1] - hsp_first[i], query_advance, target_advance, seeds[i]);
        if (!seeds[i].empty()) staged.push_back(i);
    }
    if (staged.empty()) return 0;
    std::vector<c4gpu_pair> spairs(staged.size());
    for (size_t x = 0; x < staged.size(); x++) spairs[x] = pairs[staged[x]];
    ResidentSeqs seqs;
    if (seqs.build(ctx, family, params, spairs.data(), (int)spairs.size())) return -1;
    std::vector<long long> q_off(n_pairs, 0), t_off(n_pairs, 0);
    for (size_t x = 0; x < staged.size(); x++) { q_off[staged[x]] = seqs.qoff[x]; t_off[staged[x]] = seqs.toff[x]; }
    KParams kp;
    make_kparams(model, params, &kp);
    DevBuf<KParams> d_kp;
    if (d_kp.upload(&kp, 1, ctx->stream)) return -1;
    const auto t1 = std::chrono::steady_clock::now();
    g_sdp_stats.stage_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    size_t free_b = 0, total_b = 0;
    (void)dev_mem_info(&free_b, &total_b);
    const unsigned max_chunks = (unsigned)std::min<double>(4.0e6, std::max(0.0, ((double)free_b + (double)ctx->sdp_arena_bytes) * 0.6 / CHUNK_BYTES));
    const double arena_env_mb = c4cfg::real(c4cfg::SDP_ARENA_MB, 0.0);
    std::vector<char> active(n_pairs, 0), served(n_pairs, 0);
    for (int i : staged) active[i] = 1;
    unsigned chunks = 0;
    for (int round = 0; round < 2; round++) {
        SdpHostPlan plan;
        sdp_make_plan(*fi, pairs, n_pairs, q_off, t_off, seeds, active, max_chunks, plan);
        if (plan.jobs.empty()) break;
        if (round == 0) {
            chunks = arena_env_mb > 0 ? (unsigned)(arena_env_mb * 1048576.0 / CHUNK_BYTES) : sdp_arena_guess(seeds, plan);
            if (arena_env_mb <= 0) chunks = std::max(chunks, (unsigned)(ctx->sdp_arena_bytes >> CHUNK_LOG));   // what the context already holds
        } else chunks = chunks >= max_chunks / 8 ? max_chunks : chunks * 8;
        chunks = std::min(chunks, max_chunks);
        if (chunks < 16) { c4h::set_error("SDP: no device memory for the stream arena"); return -1; }
        SdpBackendOut bo;
        unsigned chunks_used = 0;
        if (sdp_run_device(ctx, *fi, *kern, seqs, d_kp.p, plan, chunks, dropoff, threshold, bo, &g_sdp_stats.pass_ms, &g_sdp_stats.walk_ms, &chunks_used)) return -1;
        g_sdp_stats.jobs += (long long)plan.jobs.size();
        bool again = false;
        for (size_t jx = 0; jx < plan.jobs.size(); jx++) {
            const int i = plan.job_pair[jx];
            active[i] = 0;
            if (sdp_collect(*fi, model, plan, bo, (int)jx, seeds[i])) served[i] = 1;
            else if (round == 0 && chunks < max_chunks) { active[i] = 1; again = true; g_sdp_stats.reruns++; }
        }
        if (verbose) {
            size_t n_hsp = 0;
            double hsp_len = 0;
            for (size_t jx = 0; jx < plan.jobs.size(); jx++)
                for (const SdpHostSeed &h : seeds[plan.job_pair[jx]]) { n_hsp++; hsp_len += h.hsp->length; }
            fprintf(stderr, "c4gpu trace: sdp round %d: %zu jobs (%zu seeds, %.0f HSP positions), arena %u chunks of which %u taken, passes %.2f ms "
                    "walks %.2f ms (running totals)\n", round, plan.jobs.size(), n_hsp, hsp_len, chunks, chunks_used,
                    g_sdp_stats.pass_ms, g_sdp_stats.walk_ms);
        }
        if (!again) break;
    }
    const auto t2 = std::chrono::steady_clock::now();
    for (int i : staged) {
        if (!served[i]) { n_out[i] = -1; g_sdp_stats.unserved++; continue; }
        n_out[i] = sdp_single_pass(*fi, model, pairs[i], seeds[i], threshold, max_alignments, out + (size_t)i * max_alignments);
    }
    g_sdp_stats.pairs += (long long)staged.size();
    g_sdp_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
    // a small arena stays with the context (the next flush of a run is about as large); a large one goes back: the
    // Viterbi batches of the same context size their slabs by what is free
    if (!ctx->sdp_arena_keep && ctx->sdp_arena_bytes > (8ull << 30)) {
        const auto tf = std::chrono::steady_clock::now();
        (void)hipFree(ctx->sdp_arena);
        ctx->sdp_arena = nullptr; ctx->sdp_arena_bytes = 0;
        if (verbose) fprintf(stderr, "c4gpu trace: sdp arena freed in %.1f ms; host part of the batch (single-pass selection) %.1f ms\n",
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf).count(),
                             std::chrono::duration<double, std::milli>(tf - t2).count());
    }
    return 0;
  } catch (const std::exception &e) {
    c4h::set_error(std::string("c4gpu_sdp_batch: ") + e.what());
    return -1;
  }
}
