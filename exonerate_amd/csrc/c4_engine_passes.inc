// c4_engine_passes.inc -- part of c4_engine.hip (one translation unit; included there, in this order): pass scheduling below Optimal_find_path: the sequential reference route, the reduced-space route on the device (checkpoint pass -> sub-alignments -> stitch), the windowed region pass.
// ---- Optimal_find_path over a batch (optimal.c:368-413) ---------------------------------------------------------
struct Segment {                 // one Viterbi_SubAlignment (viterbi.c:482-496) in path order
    c4gpu_region region;
    int first_state;
    int final_cell[CELL_MAX];
    bool needs_checkpoints;      // Viterbi_use_reduced_space(vsa->region): recurse (optimal.c:203)
};

struct PairPlan {
    bool active = false, reduced = false;
    c4gpu_score region_score = 0;
    c4gpu_region ar;
    int end_from = 0;            // the state END was entered from in the region pass's best end cell (0: that pass did not say)
    std::vector<Segment> segs;   // reduced-space: the flattened vsa_list
};

bool model_is_global(const c4gpu_model *m) {     // C4_Model_is_global, c4.c:1959
    return m->start_scope == C4GPU_SCOPE_CORNER && m->end_scope == C4GPU_SCOPE_CORNER;
}

// Optimal_find_path_reduced_space for ONE pair exactly as the reference sequences it (optimal.c:160-345):
// every Viterbi call is its own launch and each sub-DP receives the final cell the previous one actually
// produced.  Slow path: only used when the batched prediction of those cells fails its verification.
struct SeqVsa { c4gpu_region region; int first_state; int final_cell[CELL_MAX]; };

int sequential_recur(Engine &eng, const ResidentSeqs &seqs, int pair, int dpmemory_mb, const c4gpu_region &region,
                     int first_state, const int *first_cell, int final_state, int *final_cell_out,
                     c4gpu_score *score_out, std::vector<SeqVsa> &leaves) {
    const c4gpu_model *m = eng.model;
    JobSpec js;
    js.pair = pair; js.region = region; js.first_state = first_state; js.final_state = final_state;
    memcpy(js.first_cell, first_cell, sizeof js.first_cell);
    js.cp_count = c4h::checkpoint_rows(m, &region, dpmemory_mb);
    std::vector<JobOut> outs;
    if (eng.run(seqs, MODE_CKPT, true, std::vector<JobSpec>(1, js), outs)) return -1;
    *score_out = outs[0].res.score;
    memcpy(final_cell_out, outs[0].res.final_cell, sizeof(int) * CELL_MAX);
    std::vector<SeqVsa> sub;
    for (int v = (int)outs[0].vsa.size() - 1; v >= 0; v--) {          // path order
        const DevVsa &dv = outs[0].vsa[v];
        SeqVsa sv;
        sv.region = c4gpu_region{dv.qs, dv.ts, dv.ql, dv.tl};
        sv.first_state = dv.first_state;
        memcpy(sv.final_cell, dv.final_cell, sizeof sv.final_cell);
        sub.push_back(sv);
    }
    for (size_t k = 0; k < sub.size(); k++) {
        if (c4h::use_reduced_space(m, &sub[k].region, dpmemory_mb)) {
            const int *sub_first = k ? sub[k - 1].final_cell : first_cell;
            const int sub_final_state = (k + 1 < sub.size()) ? sub[k + 1].first_state : final_state;
            c4gpu_score dummy;
            if (sequential_recur(eng, seqs, pair, dpmemory_mb, sub[k].region, sub[k].first_state, sub_first,
                                 sub_final_state, sub[k].final_cell, &dummy, leaves)) return -1;
        } else {
            leaves.push_back(sub[k]);
        }
    }
    return 0;
}

int sequential_reduced_path(Engine &eng, const ResidentSeqs &seqs, int pair, int dpmemory_mb,
                            const c4gpu_region &ar, c4gpu_alignment *a) {
    const c4gpu_model *m = eng.model;
    int zero[CELL_MAX] = {0}, final_cell[CELL_MAX];
    std::vector<SeqVsa> leaves;
    c4gpu_score score = 0;
    if (sequential_recur(eng, seqs, pair, dpmemory_mb, ar, m->start_state, zero, m->end_state, final_cell, &score,
                         leaves)) return -1;
    c4gpu_alignment_clear(a);
    a->score = score; a->region = ar; a->valid = 1;
    int cap = 0;
    for (size_t k = 0; k < leaves.size(); k++) {                      // Optimal_compute_subalignments
        JobSpec js;
        js.pair = pair; js.region = leaves[k].region; js.first_state = leaves[k].first_state;
        memcpy(js.first_cell, k ? leaves[k - 1].final_cell : zero, sizeof js.first_cell);
        js.final_state = (k + 1 < leaves.size()) ? leaves[k + 1].first_state : m->end_state;
        std::vector<JobOut> outs;
        if (eng.run(seqs, MODE_PATH, true, std::vector<JobSpec>(1, js), outs)) return -1;
        memcpy(leaves[k].final_cell, outs[0].res.final_cell, sizeof(int) * CELL_MAX);   // optimal.c:243,301
        for (uint32_t r : outs[0].runs) c4h::alignment_add(a, &cap, (int)(r >> 24), (int)(r & 0xffffff));
    }
    return 0;
}

// Steps 3 and 4 of find_path_batch for the pairs in `red` without the host in between (see fuse_expand_kernel): one
// checkpoint launch, one sub-alignment launch, one stitch; done[i] = 1 for every pair whose alignment was completed
// here.  The others (and every pair when the route does not apply) are left untouched for the host route.
// unfinished[pair]: the checkpoint pass's own result (score, final cell, sub-alignment list) of every pair the route did not
// finish, so that the host route does not run that pass again for them (a handful of whole-rectangle checkpoint jobs on a
// handful of waves takes as long as thousands: 433 ms for 11 chance alignments across 1 kb x 93 kb).
int fused_reduced_paths(Engine &eng, const ResidentSeqs &seqs, const std::vector<int> &red, const std::vector<PairPlan> &plan,
                        int dpmemory_mb, c4gpu_alignment *alignments, std::vector<char> &done, std::map<int, JobOut> &unfinished) {
    const bool trace = c4cfg::has(c4cfg::TRACE);
    const auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (trace) fprintf(stderr, "c4gpu trace:   fused: %-22s at %.3f ms\n", what,
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    };
    const c4gpu_model *m = eng.model;
    c4gpu_ctx *ctx = eng.ctx;
    const int n = (int)red.size();
    if (!n || eng.pair_sub) return 0;
    if (c4cfg::is(c4cfg::FUSED, 0)) return 0;
    const Switches sw = Switches::from_config();         // (read on every call: a test switches them)
    const int wpe_env = sw.wpe;
    long long worst = 0;
    for (int i : red) worst = std::max(worst, (long long)plan[i].ar.query_length + plan[i].ar.target_length);
    const bool cont_free = eng.cont_free_ok(worst);              // the sub-alignments lie inside their pair's region
    const KernelInfo *kc = get_kernel(eng.family, MODE_CKPT, true, cont_free, false, wpe_env, false, 0);
    const KernelInfo *kp = get_kernel(eng.family, MODE_PATH, true, cont_free, false, wpe_env, false, 0);
    if (!kc) kc = get_kernel(eng.family, MODE_CKPT, true, false, false, wpe_env, false, 0);
    if (!kp) kp = get_kernel(eng.family, MODE_PATH, true, false, false, wpe_env, false, 0);
    if (!kc || !kp) return 0;
    // the packed 16-bit checkpoint kernel (c4_ckpt16_kernel.h: two jobs per lane) for every job whose scores, checkpoint
    // payloads and intron lengths fit its halves — in its rooted form (the component of the state the path's END is entered
    // from: one strand of est2genome) where the region pass reported that state, else over every inner state;
    // C4GPU_CK16=0: never, 2..: one shape whatever the jobs (tests, measurement), C4GPU_CK16_ROOT=0: never the rooted form
    const bool ck16_on = sw.ck16 > 0 && cont_free && eng.pk16_params_ok && seqs.tdense_n > 0;      // (dense target codes: Prof16)
    const KernelInfo *kc16 = ck16_on ? get_kernel_ck16(eng.family, CK16_R4W2) : nullptr;
    const KernelInfo *kc16r = (ck16_on && sw.ck16_root) ? get_kernel_ck16(eng.family, CK16R_R6W2) : nullptr;   // its shape: chosen below
    const int ck16_tmax = c4cfg::num(c4cfg::CK16_TMAX, 0x7fffffff);      // test hook
    hipStream_t s = ctx->stream;
    const c4h::MemRule rule{m->max_query_advance, m->max_target_advance, m->n_states, m->total_shadow_designations};
    // -- the checkpoint jobs: the rooted packed kernel's first (root by root), then the packed kernel's, then the 32-bit kernel's,
    // each group longest first (persistent waves pull from the queue head)
    std::vector<int> order(n), cpn(n);
    std::vector<char> group(n, 0);                   // 2: packed, rooted; 1: packed; 0: 32-bit
    std::iota(order.begin(), order.end(), 0);
    auto cells = [&](int x) { const c4gpu_region &r = plan[red[x]].ar; return (long long)(r.query_length + 1) * (r.target_length + 1); };
    auto root_of = [&](int x) { return plan[red[x]].end_from; };
    int count_g[3] = {0, 0, 0};
    for (int x = 0; x < n; x++) {
        const c4gpu_region &r = plan[red[x]].ar;
        cpn[x] = c4h::checkpoint_rows(m, &r, dpmemory_mb);
        if (!kc16) continue;
        // payload ((row x states) + state) x max_target_advance + k in 16 bits; checkpoint columns max_target_advance apart at least
        const bool ok = eng.pk16_fits(r.query_length, r.target_length) && r.target_length <= ck16_tmax &&
                        ((long long)r.query_length + 2) * kc16->n_states * kc16->max_at <= 65535 && cpn[x] >= 1 &&
                        r.target_length / (cpn[x] + 1) >= kc16->max_at;
        group[x] = !ok ? 0 : (kc16r && root_of(x) > 1) ? 2 : 1;
        count_g[(int)group[x]]++;
    }
    for (int g = 2; g >= 1; g--)
        if (count_g[g] == 1) {                          // a lone packed job gains nothing: the group below takes it
            for (int x = 0; x < n; x++) if (group[x] == g) group[x] = (char)(g - 1);
            count_g[g - 1]++; count_g[g] = 0;
        }
    if (!count_g[1] && !count_g[2]) { kc16 = nullptr; kc16r = nullptr; }
    const int n16r = count_g[2], n16a = count_g[1], n16 = n16r + n16a;
    if (kc16r && n16r) {
        long long strips = 0;                            // of 256 rows, over the rooted jobs
        int rows_max = 0;
        for (int x = 0; x < n; x++)
            if (group[x] == 2) {
                strips += (plan[red[x]].ar.query_length + 1 + 255) / 256;
                rows_max = std::max(rows_max, plan[red[x]].ar.query_length + 1);
            }
        kc16r = get_kernel_ck16(eng.family, choose_ck16_rooted_shape(eng.family, strips, n16r, rows_max, sw));
    }
    if (n16 && eng.ensure_ss16(seqs)) return -1;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (group[a] != group[b]) return group[a] > group[b];
        if (group[a] == 2 && root_of(a) != root_of(b)) return root_of(a) < root_of(b);
        return cells(a) > cells(b);
    });
    if (c4cfg::has(c4cfg::TRACE))
        fprintf(stderr, "c4gpu trace:   fused: kernels %s, %s\nc4gpu trace:   fused: packed checkpoint kernels %s for %d, %s for %d of %d jobs\n",
                kc->name, kp->name, (kc16r && n16r) ? kc16r->name : "-", n16r, (kc16 && n16a) ? kc16->name : "-", n16a, n);
    std::vector<DevJob> &jobs = eng.hf_jobs;
    jobs.resize(n);
    long long vsa_total = 0, max_ckpt = 0, max_T = 0, ckpt_cells = 0, max_ckpt16 = 0, max_T16 = 0;
    bool carry = false, carry16 = false;
    int bnd16 = 0;
    for (int x = 0; x < n; x++) {
        const c4gpu_region &r = plan[red[order[x]]].ar;
        DevJob &j = jobs[x];
        memset(&j, 0, sizeof j);
        j.pair = red[order[x]]; j.q0 = r.query_start; j.t0 = r.target_start; j.Q = r.query_length; j.T = r.target_length;
        j.first_state = m->start_state; j.final_state = m->end_state;
        j.cp_count = cpn[order[x]];
        j.root = x < n16r ? root_of(order[x]) : 0;
        int tb = 0;
        while ((1LL << tb) <= j.T) tb++;
        j.tshift = tb;
        j.ckpt_off = -1; j.seed_off = -1;
        j.vsa_off = (int)vsa_total;
        vsa_total += j.cp_count + 1;
        ckpt_cells += (long long)(j.Q + 1) * (j.T + 1);
        if (x < n16) {
            const KernelInfo *k16 = x < n16r ? kc16r : kc16;
            max_ckpt16 = std::max(max_ckpt16, (long long)j.cp_count * k16->max_at * (j.Q + 1) * (x < n16r ? k16->ckw_root : k16->ckw));
            max_T16 = std::max<long long>(max_T16, j.T);
            bnd16 = std::max(bnd16, k16->bnd);
            if ((j.Q + 1 + 64 * k16->R - 1) / (64 * k16->R) > 1) carry16 = true;
        } else {
            max_ckpt = std::max(max_ckpt, (long long)j.cp_count * kc->max_at * (j.Q + 1) * kc->n_states * kc->cs);
            max_T = std::max<long long>(max_T, j.T);
            if ((j.Q + 1 + 64 * kc->R - 1) / (64 * kc->R) > kc->waves) carry = true;
        }
    }
    if (vsa_total > 0x7fffffffLL) return 0;
    // the packed kernels' pairs: neighbours of the same kernel and root
    std::vector<int> pair_list;
    int pairs_r = 0, pairs_a = 0;
    for (int x = 0; x < n16;) {
        const int lim = x < n16r ? n16r : n16;
        const bool two = x + 1 < lim && jobs[x + 1].root == jobs[x].root;
        pair_list.push_back(x); pair_list.push_back(two ? x + 1 : -1);
        (x < n16r ? pairs_r : pairs_a)++;
        x += two ? 2 : 1;
    }
    auto grid_for = [&](const KernelInfo *ki, long long jobs_n, long long bytes_per_wave) -> long long {
        int blocks_per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, ki->func, 64 * ki->waves, 0) != hipSuccess || blocks_per_cu < 1)
            blocks_per_cu = 1;
        long long grid = std::min<long long>(jobs_n, (long long)blocks_per_cu * ctx->prop.multiProcessorCount);
        const long long budget = (long long)(ctx->prop.totalGlobalMem / 4);
        if (bytes_per_wave * grid > budget) grid = std::max<long long>(1, budget / std::max<long long>(1, bytes_per_wave));
        return grid;
    };
    int zero = 0;
    unsigned long long zero64 = 0;
    {
        // up to three launches on the lane's stream, one after the other: they share the carry rows and the checkpoint slabs
        const int zeros[3] = {0, 0, 0};
        const int n32 = n - n16;
        const long long bnd_per_wave = (2 * ((carry ? max_T : 0) + 1) + 1) * (long long)std::max(kc->bnd, 1);
        const long long grid = n32 ? grid_for(kc, n32, bnd_per_wave * 4 + max_ckpt * 4) : 0;
        const long long bnd16_per_wave = n16 ? (2 * ((carry16 ? max_T16 : 0) + 1) + 1) * (long long)std::max(bnd16, 1) : 0;
        const long long grid16r = pairs_r ? grid_for(kc16r, pairs_r, bnd16_per_wave * 4 + 2 * max_ckpt16 * 4) : 0;
        const long long grid16a = pairs_a ? grid_for(kc16, pairs_a, bnd16_per_wave * 4 + 2 * max_ckpt16 * 4) : 0;
        const long long grid16 = std::max(grid16r, grid16a);
        if (eng.d_fjobs.upload(jobs.data(), n, s) || eng.d_fres.alloc(n) || eng.d_queue.upload(zeros, 3, s) ||
            eng.d_pairs.upload(pair_list.data(), pair_list.size(), s) ||
            eng.d_bnd.alloc(std::max(bnd_per_wave * grid, bnd16_per_wave * grid16)) || eng.d_fvsa.alloc(vsa_total) ||
            eng.d_ckpt.alloc(std::max(max_ckpt * grid, 2 * max_ckpt16 * grid16)) || eng.d_ckpt_dump.alloc(1))
            return -1;
        LaunchArgs a;
        memset(&a.scratch, 0, sizeof a.scratch);
        a.kp = eng.kparams.p; a.seqs = seqs.dev;
        a.seqs.sub_colptr = nullptr; a.seqs.sub_rows = nullptr; a.seqs.span_in = nullptr; a.seqs.span_out = nullptr;
        a.seqs.seed = nullptr;
        a.seqs.ss16 = seqs.ss16_built ? seqs.ss16.p : nullptr;
        a.vsas = eng.d_fvsa.p; a.ops = nullptr; a.stream = s;
        a.scratch.bnd = eng.d_bnd.p;
        a.scratch.ckpt_dump = eng.d_ckpt_dump.p;
        if (ctx->timing) HIP_OK(hipEventRecord(ctx->ev0, s));
        // the packed kernels index the whole job / result arrays through their pair lists
        a.jobs = eng.d_fjobs.p; a.n_jobs = n16; a.results = eng.d_fres.p;
        a.scratch.bnd_stride = bnd16_per_wave; a.scratch.carry = carry16 ? 1 : 0;
        a.scratch.ckpt = eng.d_ckpt.p; a.scratch.ckpt_stride = max_ckpt16;
        if (pairs_r || pairs_a) {
            a.seqs.sub_rows = reinterpret_cast<const int *>(seqs.tcode_dense.p);       // the packed pass's dense target codes and code
            a.seqs.sub_colptr = reinterpret_cast<const int *>(seqs.tdense.p);          // table (Prof16, c4_ckpt16_kernel.h)
        }
        if (pairs_r) {
            a.queue = eng.d_queue.p; a.grid = (int)grid16r; a.aux = eng.d_pairs.p; a.n_aux = pairs_r;
            HIP_OK(kc16r->launch(a));
        }
        if (pairs_a) {
            a.queue = eng.d_queue.p + 1; a.grid = (int)grid16a; a.aux = eng.d_pairs.p + 2 * pairs_r; a.n_aux = pairs_a;
            HIP_OK(kc16->launch(a));
        }
        a.seqs.sub_rows = nullptr; a.seqs.sub_colptr = nullptr;
        if (n32) {
            a.jobs = eng.d_fjobs.p + n16; a.n_jobs = n32; a.results = eng.d_fres.p + n16; a.queue = eng.d_queue.p + 2; a.grid = (int)grid;
            a.aux = nullptr; a.n_aux = 0;
            a.scratch.bnd_stride = bnd_per_wave; a.scratch.carry = carry ? 1 : 0;
            a.scratch.ckpt = max_ckpt ? eng.d_ckpt.p : nullptr; a.scratch.ckpt_stride = max_ckpt;
            HIP_OK(kc->launch(a));
        }
        if (ctx->timing) HIP_OK(hipEventRecord(ctx->ev1, s));
    }
    std::vector<DevResult> &res = eng.hf_res;
    res.resize(n);
    if (eng.d_fres.download(res.data(), n, s)) return -1;
    HIP_OK(c4_stream_sync(s));
    if (ctx->timing) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->kernel_ms[MODE_CKPT] += ms; ctx->kernel_launches[MODE_CKPT]++; ctx->kernel_cells[MODE_CKPT] += ckpt_cells;
    }
    lap("checkpoint pass");
    // -- the sub-alignment jobs, on the device
    std::vector<int> &first = eng.hf_first;
    first.assign(n + 1, 0);
    for (int x = 0; x < n; x++) first[x + 1] = first[x] + ((res[x].flags & FLAG_NO_END) ? 0 : res[x].n_vsa);
    const long long n_sub = first[n];
    if (!n_sub) return 0;
    std::vector<unsigned long long> stats(FUSE_STATS, 0);
    if (eng.d_ffirst.upload(first.data(), n + 1, s) || eng.d_fsub_jobs.alloc(n_sub) || eng.d_fflags.alloc(n) ||
        eng.d_fstats.upload(stats.data(), FUSE_STATS, s))
        return -1;
    if (eng.d_fflags.zero(n, s)) return -1;
    hipLaunchKernelGGL(fuse_expand_kernel, dim3(n), dim3(64), 0, s, eng.d_fjobs.p, eng.d_fvsa.p, eng.d_ffirst.p, n,
                       eng.d_fsub_jobs.p, rule, dpmemory_mb, kp->R, eng.d_fflags.p, eng.d_fstats.p,
                       (c4cfg::is(c4cfg::BYROOT, 0)) ? 0 : 1);
    HIP_OK(hipGetLastError());
    if (eng.d_fstats.download(stats.data(), FUSE_STATS, s)) return -1;
    HIP_OK(c4_stream_sync(s));
    lap("jobs listed");
    const long long max_runs = (long long)stats[FUSE_MAX_OPS_CAP], max_tb = (long long)stats[FUSE_MAX_TB];
    const long long sub_T = (long long)stats[FUSE_MAX_T], ops_total = (long long)stats[FUSE_OPS_TOTAL];
    const bool sub_carry = (long long)stats[FUSE_MAX_STRIPS] > kp->waves;
    const long long bnd_per_wave = (2 * ((sub_carry ? sub_T : 0) + 1) + 1) * (long long)std::max(kp->bnd, 1);
    const long long grid = grid_for(kp, n_sub, bnd_per_wave * 4 + max_tb * 4 + max_runs * 4);
    long long runs_capacity = std::min<long long>(ops_total, std::max<long long>(1 << 20, n_sub * 256));
    unsigned long long used = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (eng.d_fsub_res.alloc(n_sub) || eng.d_queue.upload(&zero, 1, s) || eng.d_runs_used.upload(&zero64, 1, s) ||
            eng.d_bnd.alloc(bnd_per_wave * grid) || eng.d_runs.alloc(max_runs * grid) || eng.d_runs_out.alloc(runs_capacity) ||
            eng.d_tb.alloc(max_tb * grid))
            return -1;
        LaunchArgs a;
        memset(&a.scratch, 0, sizeof a.scratch);
        a.kp = eng.kparams.p; a.seqs = seqs.dev; a.jobs = eng.d_fsub_jobs.p; a.n_jobs = (int)n_sub; a.results = eng.d_fsub_res.p;
        a.seqs.sub_colptr = nullptr; a.seqs.sub_rows = nullptr; a.seqs.span_in = nullptr; a.seqs.span_out = nullptr;
        a.seqs.seed = nullptr;
        a.vsas = nullptr; a.ops = nullptr; a.queue = eng.d_queue.p; a.grid = (int)grid; a.stream = s;
        a.scratch.bnd = eng.d_bnd.p; a.scratch.bnd_stride = bnd_per_wave; a.scratch.carry = sub_carry ? 1 : 0;
        a.scratch.tb = max_tb ? eng.d_tb.p : nullptr; a.scratch.tb_stride = max_tb;
        a.scratch.runs = eng.d_runs.p; a.scratch.runs_stride = max_runs;
        a.scratch.runs_out = eng.d_runs_out.p; a.scratch.runs_capacity = runs_capacity;
        a.scratch.runs_used = eng.d_runs_used.p;
        if (ctx->timing) HIP_OK(hipEventRecord(ctx->ev0, s));
        HIP_OK(kp->launch(a));
        if (ctx->timing) HIP_OK(hipEventRecord(ctx->ev1, s));
        if (eng.d_runs_used.download(&used, 1, s)) return -1;
        HIP_OK(c4_stream_sync(s));
        if (ctx->timing) {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            ctx->kernel_ms[MODE_PATH] += ms; ctx->kernel_launches[MODE_PATH]++;
        }
        if ((long long)used <= runs_capacity) break;
        if (attempt == 1) { c4h::set_error("traceback runs exceed their worst-case buffer"); return -1; }
        runs_capacity = ops_total;                           // rare: paths with very short runs
    }
    lap("sub-alignment pass");
    // -- verify + concatenate per pair
    if (eng.d_fout.alloc(2 * (size_t)std::max<unsigned long long>(used, 1)) || eng.d_fpairs.alloc(n) ||
        eng.d_runs_used.upload(&zero64, 1, s))
        return -1;
    hipLaunchKernelGGL(fuse_stitch_kernel, dim3((n + 63) / 64), dim3(64), 0, s, eng.d_fjobs.p, eng.d_fvsa.p, eng.d_ffirst.p, n,
                       eng.d_fsub_res.p, eng.d_runs_out.p, 1 + m->total_shadow_designations, eng.d_fflags.p, eng.d_runs_used.p,
                       eng.d_fout.p, eng.d_fpairs.p, n16, cell_strict() ? 1 : 0);
    HIP_OK(hipGetLastError());
    std::vector<FusePair> &fps = eng.hf_pairs;
    fps.resize(n);
    unsigned long long out_used = 0;
    if (eng.d_fpairs.download(fps.data(), n, s) || eng.d_runs_used.download(&out_used, 1, s)) return -1;
    HIP_OK(c4_stream_sync(s));
    std::vector<int> &out = eng.hf_out;
    out.resize(2 * (size_t)out_used);
    if (out_used) {
        if (eng.d_fout.download(out.data(), 2 * (size_t)out_used, s)) return -1;
        HIP_OK(c4_stream_sync(s));
    }
    lap("stitched + downloaded");
    int n_done = 0;
    for (int x = 0; x < n; x++) {
        if (fps[x].status & 1) continue;
        const int i = red[order[x]];
        c4gpu_alignment &a = alignments[i];
        a.score = res[x].score;
        a.region = plan[i].ar;
        a.valid = 1;
        a.n_ops = fps[x].count;
        if (a.n_ops) {
            a.op_transition = (int32_t *)malloc(sizeof(int32_t) * a.n_ops);
            a.op_length = (int32_t *)malloc(sizeof(int32_t) * a.n_ops);
            const int *src = out.data() + 2 * fps[x].off;
            for (int k = 0; k < a.n_ops; k++) { a.op_transition[k] = src[2 * k]; a.op_length[k] = src[2 * k + 1]; }
        }
        done[i] = 1;
        n_done++;
    }
    if (n_done < n) {
        std::vector<DevVsa> vsa((size_t)vsa_total);
        if (eng.d_fvsa.download(vsa.data(), vsa_total, s)) return -1;
        HIP_OK(c4_stream_sync(s));
        for (int x = 0; x < n; x++) {
            if (!(fps[x].status & 1)) continue;
            JobOut o;
            o.res = res[x];
            o.runs.n = 0;
            o.packed = x < n16;
            if (!(res[x].flags & FLAG_NO_END)) o.vsa.assign(vsa.begin() + jobs[x].vsa_off, vsa.begin() + jobs[x].vsa_off + res[x].n_vsa);
            unfinished[red[order[x]]] = std::move(o);
        }
    }
    if (c4cfg::has(c4cfg::TRACE))
    {
        long long score_only = 0;
        for (int x = 0; x < n; x++) score_only += fps[x].status >> 8;
        fprintf(stderr, "c4gpu trace:   fused: %d of %d pairs finished on the device route, %lld sub-alignments, %lld final cells that "
                "differ from their prediction in the score only\n", n_done, n, n_sub, score_only);
    }
    lap("alignments built");
    return 0;
}

// FIND_REGION of whole rectangles in two passes (c4_viterbi_kernel.h, SEED): a score pass that also dumps the DP state
// every K columns, then region-start payload passes over windows of one dump interval each, walking left from the end
// cell until the payload is a real start.  Scores, end cells and starts are those of the one-pass kernel (every
// window cell is computed from the whole-rectangle pass's own values); the payload work shrinks from the whole target
// to the alignment's extent.  out[x] for pairs[x]: score, qe, te always; qs, ts where the score reaches thr(pair).
template <class Thr>
int windowed_region_pass(Engine &eng, const ResidentSeqs &seqs, const std::vector<int> &pairs,
                         const std::vector<PairPlan> &plan, Thr thr, int kshift, std::vector<DevResult> &out) {
    const int n = (int)pairs.size();
    auto nbits = [](int v) { int b = 0; while ((1LL << b) <= v) b++; return b; };
    std::vector<JobSpec> specs(n);
    std::vector<JobOut> outs;
    for (int x = 0; x < n; x++) { specs[x].pair = pairs[x]; specs[x].region = plan[pairs[x]].ar; }
    SeedPlan sp1;
    sp1.mode = 1; sp1.kshift = kshift;
    if (eng.run(seqs, MODE_SCORE, false, specs, outs, &sp1)) return -1;
    const long long seedw = sp1.seedw;                   // ints per dumped row: the score kernel's format (32-bit cells or Dump16)
    const int dc = sp1.dc;                               // dumped columns per dump (d*K - (dc - 1) .. d*K)
    out.assign(n, DevResult());
    // the windows of a pair follow each other inside one workgroup (viterbi_kernel_mw, SEED 2): ONE launch over the first
    // windows of all wanted pairs; a job walks left from the end cell, one dump interval per window, until its payload is a
    // real start or its hop budget is spent
    std::vector<int> want;
    for (int x = 0; x < n; x++) {
        out[x] = outs[x].res;
        out[x].qs = out[x].ts = 0;
        if (!outs[x].res.end_set || outs[x].res.score < thr(pairs[x])) continue;
        want.push_back(x);
    }
    const size_t wanted = want.size();
    // hop budget: enough windows for the longest way back any wanted pair can have (a path that starts in the first dump
    // interval: reverse strands of the north-star batch, 289 of 1 024 pairs at 12 hops -- the one-pass kernel that finished
    // them cost 127 ms per 1 024 pairs, the extra hops cost nothing: profiles/r03_step.md), at least 12, at most 64
    int need_hops = 12;
    for (int x : want) need_hops = std::max(need_hops, ((outs[x].res.te - 1) >> kshift) + 2);
    const int max_hops = c4cfg::num(c4cfg::WINDOW_HOPS, std::min(need_hops, 64));
    std::vector<int> open;                                       // pairs whose path runs back further than the hop budget
    std::vector<char> demoted(n, 0);                             // ... and pairs the packed route could not serve (below)
    long long windows = 0;
    // C4GPU_STRICT=1 (debugging): a packed pass that disagrees with the 32-bit kernels fails the call instead of handing the
    // pair to them; C4GPU_FORCE_CORNER_MISMATCH=k (test hook): every k-th wanted pair is treated as such a disagreement
    const bool strict = c4cfg::nonzero(c4cfg::STRICT);
    const int force_miss = c4cfg::num(c4cfg::FORCE_CORNER_MISMATCH, 0);
    if (sp1.fmt16) {
        // the packed windows compute the component of the state END was entered from (DevResult::last_srp of the score pass);
        // a pair without one goes to the one-pass 32-bit kernel, which needs none
        std::vector<int> keep;
        for (int x : want) {
            if (outs[x].res.last_srp > 1) { keep.push_back(x); continue; }
            if (strict) { c4h::set_error("windowed region pass: the score pass did not say where END was entered from"); return -1; }
            if (c4cfg::has(c4cfg::TRACE)) fprintf(stderr, "c4gpu trace:   pair %d: no root from the packed score pass, one-pass kernel\n", pairs[x]);
            open.push_back(x); demoted[x] = 1;
        }
        want.swap(keep);
    }
    if (!want.empty()) {
        std::vector<JobSpec> hs(want.size());
        SeedPlan sp2;
        sp2.mode = 2; sp2.kshift = kshift; sp2.hops = std::max(1, max_hops); sp2.fmt16 = sp1.fmt16;
        sp2.off.resize(want.size()); sp2.rows.resize(want.size()); sp2.base.resize(want.size());
        sp2.d.resize(want.size()); sp2.t0w.resize(want.size()); sp2.t0_base.resize(want.size());
        for (size_t h = 0; h < want.size(); h++) {
            const int x = want[h];
            const c4gpu_region &ar = plan[pairs[x]].ar;
            const int d = (outs[x].res.te - 1) >> kshift;
            const int t0w = d >= 1 ? (d << kshift) - (dc - 1) : 0;      // window column 0 = lattice column t0w
            hs[h].pair = pairs[x];
            hs[h].region = c4gpu_region{ar.query_start, ar.target_start + t0w, outs[x].res.qe, outs[x].res.te - t0w};
            hs[h].final_state = eng.model->end_state;
            if (sp1.fmt16) {
                // the packed windows compute the component of the state END was entered from, and end in that state
                // (the score pass reports it: DevResult::last_srp)
                hs[h].final_state = hs[h].root = outs[x].res.last_srp;
            }
            sp2.rows[h] = ar.query_length + 1;
            sp2.base[h] = sp1.off[x];
            sp2.off[h] = d >= 1 ? sp1.off[x] + (long long)(d - 1) * dc * (ar.query_length + 1) * seedw : -1;
            sp2.d[h] = d; sp2.t0w[h] = t0w; sp2.t0_base[h] = ar.target_start;
        }
        std::vector<JobOut> wouts;
        if (eng.run(seqs, MODE_REGION, false, hs, wouts, &sp2)) return -1;
        for (size_t h = 0; h < want.size(); h++) {
            const DevResult &r = wouts[h].res;
            DevResult &o = out[want[h]];
            if (!r.end_set || r.score != o.score || (force_miss > 0 && h % (size_t)force_miss == 0)) {
                // never seen outside the test hook; should a packed pass ever disagree with itself, the pair is the one-pass
                // 32-bit kernel's (the other pairs of the call keep their results)
                if (c4cfg::has(c4cfg::TRACE))
                    fprintf(stderr, "c4gpu trace:   pair %d: score pass %d at (%d, %d), window corner %d (set %d): one-pass kernel\n", pairs[want[h]],
                            o.score, o.qe, o.te, r.score, (int)r.end_set);
                if (strict) { c4h::set_error("windowed region pass: a window's corner cell differs from the score pass"); return -1; }
                open.push_back(want[h]); demoted[want[h]] = 1;
                continue;
            }
            windows += r.n_vsa;
            if (r.pad >= 0) { o.qs = r.qs; o.ts = r.ts; }
            else open.push_back(want[h]);
        }
    }
    if (!open.empty()) {
        // the one-pass kernel over their whole rectangles finishes them (same result: it is what the windows reproduce
        // piece by piece)
        std::vector<JobSpec> fs(open.size());
        for (size_t h = 0; h < open.size(); h++) { fs[h].pair = pairs[open[h]]; fs[h].region = plan[pairs[open[h]]].ar; }
        if (eng.run(seqs, MODE_REGION, false, fs, outs)) return -1;
        for (size_t h = 0; h < open.size(); h++) {
            const DevResult &r = outs[h].res;
            DevResult &o = out[open[h]];
            if (r.score != o.score || r.qe != o.qe || r.te != o.te) {
                if (c4cfg::has(c4cfg::TRACE))
                    fprintf(stderr, "c4gpu trace:   pair %d: score pass %d at (%d, %d), one-pass kernel %d at (%d, %d)\n", pairs[open[h]],
                            o.score, o.qe, o.te, r.score, r.qe, r.te);
                if (strict || !demoted[open[h]]) {
                    c4h::set_error("windowed region pass: the one-pass kernel disagrees with the score pass");
                    return -1;
                }
                // a pair the packed route gave up on: the one-pass 32-bit kernel's result stands
                o = r;
            }
            o.qs = r.qs; o.ts = r.ts;
            if (demoted[open[h]]) o.last_srp = 0;       // "root not known": the checkpoint pass takes its unrooted / 32-bit form
        }
    }
    const std::vector<int> &hops = open;
    const long long round = windows;
    if (wanted >= 64 && !force_miss) {
        const double rate = 1.0 - (double)hops.size() / (double)wanted;
        eng.ctx->window_rate = eng.ctx->window_rate < 0 ? rate : 0.5 * eng.ctx->window_rate + 0.5 * rate;
    }
    if (c4cfg::has(c4cfg::TRACE))
        fprintf(stderr, "c4gpu trace: windowed region pass: %d pairs, dumps every %d columns, %lld windows in one launch, %zu of %zu "
                "paths left to the one-pass kernel\n", n, 1 << kshift, round, hops.size(), wanted);
    return 0;
}

