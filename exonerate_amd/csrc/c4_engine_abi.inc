// c4_engine_abi.inc -- part of c4_engine.hip (one translation unit; included there, in this order): the C ABI of include/c4gpu.h: contexts, batches, stages, raw Viterbi calls.
// ---- the C ABI --------------------------------------------------------------------------------------------------
struct c4gpu_batch {
    c4gpu_ctx *ctx;
    c4gpu_model model;
    c4gpu_params params;
    Engine eng;
    ResidentSeqs seqs;
    std::vector<c4gpu_score> scores;
    std::vector<c4gpu_region> regions;
    std::vector<c4gpu_alignment> alignments;
    // the sub-optimal loop (c4gpu_batch_next_paths): one SubOpt per pair, pairs still in the loop
    std::vector<c4gpu_subopt *> subopts;
    std::vector<uint8_t> in_loop;
    std::vector<c4gpu_score> pair_thresholds;        // c4gpu_batch_set_thresholds; empty = none
    // engines of further models run on the same resident sequences (c4gpu_batch_viterbi_model): BSDP's derived
    // terminal / join / span models of the batch's model, keyed by the flattened model's bytes
    struct ExtraEngine { c4gpu_model model; Engine eng; };
    std::map<std::string, std::unique_ptr<ExtraEngine>> extra;
    std::unique_ptr<SideLane> side;                  // the second launch lane of large batches (find_path_lanes), made on first use
    bool annotation_applied = false;                 // c4gpu_batch_set_annotation: the query codes on the device carry CDS positions
    void clear_loop() {
        for (c4gpu_subopt *so : subopts) c4gpu_subopt_destroy(so);
        subopts.clear(); in_loop.clear();
    }
};

// The next batch on its way to the device while the current one is aligned (c4gpu_stage_load on one thread, c4gpu_batch_run
// on another): its own stream (non-blocking: no implicit synchronisation with the streams the passes run on), its own
// engine for the parameter block the packed splice array is built from, page-locked host buffers and device arrays that the
// batch it is swapped into hands back for the batch after.
struct c4gpu_stage {
    c4gpu_ctx ctx;
    c4gpu_model model;
    c4gpu_params params;
    Engine eng;
    ResidentSeqs seqs;
    bool loaded = false;
    double load_ms = 0;
    ~c4gpu_stage() {
        if (ctx.stream) (void)hipStreamDestroy(ctx.stream);
        if (ctx.ev0) (void)hipEventDestroy(ctx.ev0);
        if (ctx.ev1) (void)hipEventDestroy(ctx.ev1);
    }
};

extern "C" {

int c4gpu_abi_version(void) { return C4GPU_ABI_VERSION; }
int c4gpu_config_reload(void) {
    (void)c4cfg::get();                       // (the once-flag is spent before the table is written again)
    c4cfg::load_from_environment();
    int n = 0;
    for (int k = 0; k < c4cfg::N_KEYS; k++) n += c4cfg::table().e[k].set ? 1 : 0;
    return n;
}
const char *c4gpu_last_error(void) { return c4h::g_error.c_str(); }

static std::atomic<int> g_warm_cancel{0};        // c4gpu_ctx_warm_cancel; reset by every c4gpu_ctx_create

c4gpu_ctx *c4gpu_ctx_create(int device_ordinal) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        c4h::set_error(std::string("no HIP device available (") + hipGetErrorString(e) +
                       "): libc4gpu has no CPU fallback");
        return nullptr;
    }
    if (device_ordinal < 0 || device_ordinal >= count) { c4h::set_error("bad device ordinal"); return nullptr; }
    g_warm_cancel.store(0, std::memory_order_relaxed);       // a cancelled warm-up belongs to the context that was being left
    c4gpu_ctx *ctx = new c4gpu_ctx;
    ctx->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess || hipGetDeviceProperties(&ctx->prop, device_ordinal) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        c4h::set_error("cannot initialise the HIP device");
        delete ctx;
        return nullptr;
    }
    if (!strstr(ctx->prop.gcnArchName, "gfx950")) {
        c4h::set_error(std::string("device is ") + ctx->prop.gcnArchName + ", kernels are built for gfx950 only");
        delete ctx;
        return nullptr;
    }
    g_retired.set_cap_for(ctx->prop.totalGlobalMem);
    return ctx;
}

int c4gpu_model_device_family(const c4gpu_model *model) { return model_family(*model); }

int c4gpu_packed_route_fits(const c4gpu_model *model, const c4gpu_params *params, int32_t query_length, int32_t target_length) {
    std::unique_ptr<Engine> eng(new Engine);
    std::unique_ptr<KParams> kp(new KParams);
    if (eng->init_host(nullptr, model, params, *kp)) return -1;
    return (eng->pk16_params_ok && eng->family == FAM_EST2GENOME && eng->pk16_fits(query_length, target_length)) ? 1 : 0;
}

int c4gpu_loop_sections(const c4gpu_model *model, const c4gpu_params *params, int32_t *loop_transition, int32_t n_states) {
    std::unique_ptr<Engine> eng(new Engine);
    std::unique_ptr<KParams> kp(new KParams);
    if (eng->init_host(nullptr, model, params, *kp)) return -1;
    int found = 0;
    for (int s = 0; s < n_states; s++) {
        loop_transition[s] = s < 16 ? kp->loop_tr[s] : -1;
        found += loop_transition[s] >= 0;
    }
    return found;
}

int c4gpu_memrule_device(c4gpu_ctx *ctx, const c4gpu_model *model, int dpmemory_mb, const int32_t *query_length,
                         const int32_t *target_length, int32_t n, int32_t *reduced, int32_t *rows) {
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    DevBuf<int> dq, dt, dr, dw;
    hipStream_t s = ctx->stream;
    const c4h::MemRule rule{model->max_query_advance, model->max_target_advance, model->n_states, model->total_shadow_designations};
    if (dq.upload(query_length, n, s) || dt.upload(target_length, n, s) || dr.alloc(n) || dw.alloc(n)) return -1;
    hipLaunchKernelGGL(memrule_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, s, rule, dpmemory_mb, dq.p, dt.p, n, dr.p, dw.p);
    HIP_OK(hipGetLastError());
    if (dr.download(reduced, n, s) || dw.download(rows, n, s)) return -1;
    HIP_OK(c4_stream_sync(s));
    return 0;
}

// Load the code objects a heuristic run touches first (sequence preparation, HSP extension, word scan; the SDP passes of
// every family) without launching anything: hipFuncGetAttributes resolves a kernel, which loads its translation unit's
// code object.  Meant for a background thread while the host still reads sequences (the drop-in: c4gpu_shim.c).
// c4gpu_ctx_warm_cancel(): a warm-up that is running (on whatever thread) returns before its next load, one that has not
// started loads nothing -- so that a caller that is about to leave can join its warm-up thread within one load (the drop-in's
// way out, integration/c4gpu_shim.c: no thread is inside the HIP runtime when the exit handlers run).
void c4gpu_ctx_warm_cancel(void) { g_warm_cancel.store(1, std::memory_order_relaxed); }
void c4gpu_ctx_warm(c4gpu_ctx *ctx) {
    if (!ctx || g_warm_cancel.load(std::memory_order_relaxed) || hipSetDevice(ctx->device) != hipSuccess) return;
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, (const void *)encode_kernel);
    const c4sdp::SdpKernels *ks[4] = {c4sdp::sdp_kernels_affine(), c4sdp::sdp_kernels_protein2dna(), c4sdp::sdp_kernels_est2genome(),
                                      c4sdp::sdp_kernels_protein2genome()};
    for (const c4sdp::SdpKernels *k : ks) {
        if (g_warm_cancel.load(std::memory_order_relaxed)) break;
        (void)hipFuncGetAttributes(&a, k->rev_func);
        if (g_warm_cancel.load(std::memory_order_relaxed)) break;
        (void)hipFuncGetAttributes(&a, k->fwd_func);
    }
    (void)hipGetLastError();
}

void c4gpu_ctx_destroy(c4gpu_ctx *ctx) {
    if (!ctx) return;
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->sdp_arena) (void)hipFree(ctx->sdp_arena);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    g_retired.flush();
}

void c4gpu_ctx_set_stream(c4gpu_ctx *ctx, void *hip_stream) {
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->owns_stream = false;
    ctx->stream = (hipStream_t)hip_stream;
}

int c4gpu_ctx_sdp_reserve(c4gpu_ctx *ctx, int64_t bytes) {
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("c4gpu_ctx_sdp_reserve: cannot select the device"); return -1; }
    if (bytes <= 0) {
        ctx->sdp_arena_keep = false;
        if (ctx->sdp_arena) (void)hipFree(ctx->sdp_arena);
        ctx->sdp_arena = nullptr; ctx->sdp_arena_bytes = 0;
        return 0;
    }
    size_t free_b = 0, total_b = 0;
    if (dev_mem_info(&free_b, &total_b) != hipSuccess) { c4h::set_error("c4gpu_ctx_sdp_reserve: hipMemGetInfo failed"); return -1; }
    size_t want = std::min<size_t>((size_t)bytes, (size_t)((double)(free_b + ctx->sdp_arena_bytes) * 0.6));
    want &= ~(((size_t)1 << 16) - 1);                     // whole 64 KB chunks
    ctx->sdp_arena_keep = true;
    if (ctx->sdp_arena_bytes >= want) return 0;
    if (ctx->sdp_arena) (void)hipFree(ctx->sdp_arena);
    ctx->sdp_arena = nullptr; ctx->sdp_arena_bytes = 0;
    if (dev_malloc(&ctx->sdp_arena, want) != hipSuccess) {
        (void)hipGetLastError();
        ctx->sdp_arena = nullptr;
        c4h::set_error("c4gpu_ctx_sdp_reserve: allocation failed");
        return -1;
    }
    ctx->sdp_arena_bytes = want;
    return 0;
}

int c4gpu_ctx_own_stream(c4gpu_ctx *ctx) {
    if (ctx->owns_stream) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("c4gpu_ctx_own_stream: cannot select the device"); return -1; }
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        c4h::set_error("c4gpu_ctx_own_stream: cannot create a stream");
        return -1;
    }
    ctx->stream = s;
    ctx->owns_stream = true;
    return 0;
}

int c4gpu_ctx_device_info(c4gpu_ctx *ctx, char *name, size_t name_len, int *n_cu, int64_t *mem_bytes) {
    if (name && name_len) snprintf(name, name_len, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    if (n_cu) *n_cu = ctx->prop.multiProcessorCount;
    if (mem_bytes) *mem_bytes = (int64_t)ctx->prop.totalGlobalMem;
    return 0;
}

int c4gpu_splice_predict(c4gpu_ctx *ctx, const c4gpu_params *params, const uint8_t *target, int32_t target_len,
                         int32_t *out[4]) {
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    c4gpu_pair pair{(const uint8_t *)"A", 1, target, target_len};
    ResidentSeqs seqs;
    if (seqs.build(ctx, FAM_EST2GENOME, params, &pair, 1)) return -1;
    for (int k = 0; k < 4; k++) {
        HIP_OK(hipMemcpyAsync(out[k], seqs.ss.p + (long long)k * seqs.dev.ss_stride, sizeof(int) * (size_t)target_len,
                              hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_OK(c4_stream_sync(ctx->stream));
    return 0;
}

}  // extern "C"

static int viterbi_jobs(Engine &eng, const ResidentSeqs &seqs, int mode, const c4gpu_viterbi_job *jobs,
                        int32_t n_jobs, c4gpu_viterbi_result *results) {
    // jobs with and without continuation run different kernels (the model copy with CORNER scopes)
    for (int cont = 0; cont < 2; cont++) {
        std::vector<JobSpec> specs;
        std::vector<int> idx;
        for (int i = 0; i < n_jobs; i++) {
            if ((jobs[i].use_continuation != 0) != (cont != 0)) continue;
            JobSpec s;
            s.pair = jobs[i].pair; s.region = jobs[i].region;
            s.first_state = jobs[i].continuation.first_state; s.final_state = jobs[i].continuation.final_state;
            for (int l = 0; l < CELL_MAX; l++) s.first_cell[l] = jobs[i].continuation.first_cell[l];
            s.cp_count = jobs[i].checkpoint_count;
            s.dump_checkpoints = (mode == C4GPU_MODE_FIND_CHECKPOINTS);
            s.sub = jobs[i].subopt;
            s.span_in = jobs[i].start_cells; s.span_out = jobs[i].end_cells;
            specs.push_back(s); idx.push_back(i);
        }
        if ((mode == C4GPU_MODE_FIND_CHECKPOINTS || mode == C4GPU_MODE_FIND_REGION) && !specs.empty() &&
            ((mode == C4GPU_MODE_FIND_CHECKPOINTS) != (cont != 0))) {
            c4h::set_error("FIND_CHECKPOINTS runs with a continuation, FIND_REGION without (optimal.c:47-68)");
            return -1;
        }
        std::vector<JobOut> outs;
        if (eng.run(seqs, mode, cont != 0, specs, outs)) return -1;
        for (size_t x = 0; x < idx.size(); x++) {
            c4gpu_viterbi_result &r = results[idx[x]];
            const DevResult &d = outs[x].res;
            memset(&r, 0, sizeof r);
            r.score = d.score; r.query_start = d.qs; r.target_start = d.ts; r.query_end = d.qe; r.target_end = d.te;
            for (int l = 0; l < CELL_MAX; l++) r.final_cell[l] = d.final_cell[l];
            r.last_srp = d.last_srp;
            r.n_ops = 0;
            for (uint32_t run : outs[x].runs) r.n_ops += (int)(run & 0xffffff);
            if (r.n_ops) {
                r.ops = (int32_t *)malloc(sizeof(int32_t) * r.n_ops);
                int k = 0;
                for (uint32_t run : outs[x].runs)
                    for (uint32_t c = 0; c < (run & 0xffffff); c++) r.ops[k++] = (int)(run >> 24);
            }
            if (!outs[x].checkpoints.empty()) {
                r.checkpoints = (c4gpu_score *)malloc(sizeof(int) * outs[x].checkpoints.size());
                memcpy(r.checkpoints, outs[x].checkpoints.data(), sizeof(int) * outs[x].checkpoints.size());
            }
        }
    }
    return 0;
}


extern "C" {

int c4gpu_viterbi_batch(c4gpu_ctx *ctx, const c4gpu_model *model, const c4gpu_params *params, int mode,
                        const c4gpu_pair *pairs, int32_t n_pairs, const c4gpu_viterbi_job *jobs, int32_t n_jobs,
                        c4gpu_viterbi_result *results) {
    try {
        if (hipSetDevice(ctx->device) != hipSuccess) return -1;
        Engine eng;
        ResidentSeqs seqs;
        if (eng.init(ctx, model, params) || seqs.build(ctx, eng.family, params, pairs, n_pairs)) return -1;
        return viterbi_jobs(eng, seqs, mode, jobs, n_jobs, results);
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_viterbi_batch: ") + e.what());
        return -1;
    }
}

int c4gpu_batch_viterbi(c4gpu_batch *b, int mode, const c4gpu_viterbi_job *jobs, int32_t n_jobs,
                        c4gpu_viterbi_result *results) {
    try {
        if (hipSetDevice(b->ctx->device) != hipSuccess) return -1;
        return viterbi_jobs(b->eng, b->seqs, mode, jobs, n_jobs, results);
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_batch_viterbi: ") + e.what());
        return -1;
    }
}

int c4gpu_batch_viterbi_model(c4gpu_batch *b, const c4gpu_model *model, int mode, const c4gpu_viterbi_job *jobs,
                              int32_t n_jobs, c4gpu_viterbi_result *results) {
    try {
        if (hipSetDevice(b->ctx->device) != hipSuccess) return -1;
        const std::string key(reinterpret_cast<const char *>(model), sizeof(c4gpu_model));
        auto it = b->extra.find(key);
        if (it == b->extra.end()) {
            std::unique_ptr<c4gpu_batch::ExtraEngine> e(new c4gpu_batch::ExtraEngine);
            e->model = *model;
            // an annotated batch's codes carry row 24: the other model's engine arms the same veto row and guards
            // (c4gpu_batch_set_annotation drops these engines whenever that changes)
            e->eng.annotated = b->eng.annotated;
            if (e->eng.init(b->ctx, &e->model, &b->params)) return -1;
            // the resident arrays were prepared for the batch's own model: the other model must read the same ones
            if (family_is_p2d(e->eng.family) != family_is_p2d(b->eng.family) || family_is_codon(e->eng.family) != family_is_codon(b->eng.family) ||
                (family_has_splice(e->eng.family) && !family_has_splice(b->eng.family)) ||
                (family_has_phase(e->eng.family) && !family_has_phase(b->eng.family)) ||
                // the two codon models share their arrays' layout but not their derived models: coding2coding's on a
                // coding2genome batch is a caller's mistake (the other way round fails the splice test above)
                (family_is_coding2coding(e->eng.family) && family_is_coding2genome(b->eng.family))) {
                c4h::set_error(std::string("model [") + model->name + "] needs sequence arrays this batch was not built with");
                return -1;
            }
            it = b->extra.emplace(key, std::move(e)).first;
        }
        return viterbi_jobs(it->second->eng, b->seqs, mode, jobs, n_jobs, results);
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_batch_viterbi_model: ") + e.what());
        return -1;
    }
}

void c4gpu_viterbi_result_clear(c4gpu_viterbi_result *r) {
    free(r->ops);
    free(r->checkpoints);
    r->ops = nullptr; r->checkpoints = nullptr;
}

static int score_pass(Engine &eng, const ResidentSeqs &seqs, int mode, std::vector<JobOut> &outs) {
    std::vector<JobSpec> specs(seqs.n_pairs);
    for (int i = 0; i < seqs.n_pairs; i++) {
        specs[i].pair = i;
        specs[i].region = c4gpu_region{0, 0, seqs.qlen[i], seqs.tlen[i]};
    }
    return eng.run(seqs, mode, false, specs, outs);
}

int c4gpu_optimal_find_score_batch(c4gpu_ctx *ctx, const c4gpu_model *model, const c4gpu_params *params,
                                   const c4gpu_pair *pairs, int32_t n_pairs, c4gpu_score *scores) {
    try {
        if (hipSetDevice(ctx->device) != hipSuccess) return -1;
        Engine eng;
        ResidentSeqs seqs;
        std::vector<JobOut> outs;
        if (eng.init(ctx, model, params) || seqs.build(ctx, eng.family, params, pairs, n_pairs) ||
            score_pass(eng, seqs, MODE_SCORE, outs)) return -1;
        for (int i = 0; i < n_pairs; i++) scores[i] = outs[i].res.score;
        return 0;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_optimal_find_score_batch: ") + e.what());
        return -1;
    }
}

int c4gpu_optimal_find_path_batch(c4gpu_ctx *ctx, const c4gpu_model *model, const c4gpu_params *params,
                                  const c4gpu_pair *pairs, int32_t n_pairs, int dpmemory_mb, c4gpu_score threshold,
                                  c4gpu_alignment *alignments) {
    try {
        if (hipSetDevice(ctx->device) != hipSuccess) return -1;
        Engine eng;
        ResidentSeqs seqs;
        if (eng.init(ctx, model, params) || seqs.build(ctx, eng.family, params, pairs, n_pairs)) return -1;
        SideLane side;
        const bool two = lanes_wanted(seqs, nullptr, false);
        if (two && side.init(ctx, model, params)) return -1;
        return find_path_lanes(eng, two ? &side : nullptr, seqs, dpmemory_mb, threshold, alignments);
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_optimal_find_path_batch: ") + e.what());
        return -1;
    }
}

int c4gpu_optimal_find_path_batch_subopt(c4gpu_ctx *ctx, const c4gpu_model *model, const c4gpu_params *params,
                                         const c4gpu_pair *pairs, int32_t n_pairs, int dpmemory_mb,
                                         c4gpu_score threshold, const c4gpu_subopt *const *subopts,
                                         const uint8_t *active, c4gpu_alignment *alignments) {
    try {
        if (hipSetDevice(ctx->device) != hipSuccess) return -1;
        Engine eng;
        ResidentSeqs seqs;
        if (eng.init(ctx, model, params) || seqs.build(ctx, eng.family, params, pairs, n_pairs)) return -1;
        std::vector<const c4gpu_subopt *> subs(n_pairs, nullptr);
        if (subopts) for (int i = 0; i < n_pairs; i++) subs[i] = subopts[i];
        return find_path_batch(eng, seqs, dpmemory_mb, threshold, alignments, &subs, active);
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_optimal_find_path_batch_subopt: ") + e.what());
        return -1;
    }
}

c4gpu_batch *c4gpu_batch_create(c4gpu_ctx *ctx, const c4gpu_model *model, const c4gpu_params *params,
                                const c4gpu_pair *pairs, int32_t n_pairs) {
    try {
        if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
        c4gpu_batch *b = new c4gpu_batch;
        b->ctx = ctx; b->model = *model; b->params = *params;
        if (b->eng.init(ctx, &b->model, &b->params) || b->seqs.build(ctx, b->eng.family, &b->params, pairs, n_pairs)) {
            delete b;
            return nullptr;
        }
        return b;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_batch_create: ") + e.what());
        return nullptr;
    }
}

void c4gpu_batch_destroy(c4gpu_batch *b) {
    if (!b) return;
    b->clear_loop();
    for (auto &a : b->alignments) c4gpu_alignment_clear(&a);
    delete b;
    g_retired.flush();
}

c4gpu_stage *c4gpu_stage_create(c4gpu_ctx *ctx, const c4gpu_model *model, const c4gpu_params *params) {
    try {
        if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
        std::unique_ptr<c4gpu_stage> st(new c4gpu_stage);
        st->ctx.device = ctx->device; st->ctx.prop = ctx->prop;
        st->model = *model; st->params = *params;
        // lowest priority: the passes of the batch that is running get the compute units first, the staging kernels fill
        // what their tails leave idle (a load has a whole step's time)
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        if (hipStreamCreateWithPriority(&st->ctx.stream, hipStreamNonBlocking, prio_least) != hipSuccess ||
            hipEventCreate(&st->ctx.ev0) != hipSuccess || hipEventCreate(&st->ctx.ev1) != hipSuccess) {
            c4h::set_error("c4gpu_stage_create: cannot create the staging stream");
            return nullptr;
        }
        if (st->eng.init(&st->ctx, &st->model, &st->params)) return nullptr;
        if (c4_stream_sync(st->ctx.stream) != hipSuccess) return nullptr;
        return st.release();
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_stage_create: ") + e.what());
        return nullptr;
    }
}

int c4gpu_stage_load(c4gpu_stage *st, const c4gpu_pair *pairs, int32_t n_pairs) {
    try {
        if (hipSetDevice(st->ctx.device) != hipSuccess) return -1;
        const auto t0 = std::chrono::steady_clock::now();
        st->loaded = false;
        // the packed passes' splice array: written by the splice kernel itself here (ss16_kernel's formula with the calc
        // constants of the pre-splice transitions as `fold`), where the first packed launch would otherwise build it inside
        // the step (C4GPU_PK16=0: no packed pass, no array)
        const bool pk = pk16_enabled(st->eng.family, st->eng.pk16_params_ok, n_pairs, Switches::from_config());
        SpliceFold fold{{0, 0, 0, 0}};
        for (int i = 0; i < st->model.n_calcs; i++)
            if (st->model.calcs[i].kind == C4GPU_CALC_SPLICE_PRE) fold.add[st->model.calcs[i].param & 3] = st->model.calcs[i].value;
            else if (st->model.calcs[i].kind == C4GPU_CALC_SPLICE_POST) fold.add[st->model.calcs[i].param & 3] = 0;
        if (st->seqs.build(&st->ctx, st->eng.family, &st->params, pairs, n_pairs, true, pk ? &fold : nullptr)) return -1;
        if (pk && st->eng.ensure_ss16(st->seqs)) return -1;            // (only where the tiled splice kernel did not run)
        if (pk && c4cfg::has(c4cfg::SS16_CHECK)) {
            // test hook: the array the splice kernel wrote against the one ss16_kernel builds from the int arrays
            DevBuf<uint2> chk;
            const size_t nn = (size_t)st->seqs.ss_len;
            if (chk.alloc(nn)) return -1;
            HIP_OK(pk16_build_splice(st->eng.family, st->eng.kparams.p, st->seqs.dev.ss, st->seqs.dev.ss_stride, st->seqs.ss_len, chk.p, st->ctx.stream));
            std::vector<uint2> a(nn), b(nn);
            if (chk.download(a.data(), nn, st->ctx.stream) || st->seqs.ss16.download(b.data(), nn, st->ctx.stream)) return -1;
            HIP_OK(c4_stream_sync(st->ctx.stream));
            for (int i = 0; i < st->seqs.n_pairs; i++)
                for (long long x = st->seqs.toff[i]; x < st->seqs.toff[i] + st->seqs.tlen[i]; x++)
                    if (a[x].x != b[x].x || a[x].y != b[x].y) {
                        c4h::set_error("C4GPU_SS16_CHECK: the fused packed splice array differs from ss16_kernel's");
                        return -1;
                    }
        }
        st->loaded = true;
        st->load_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_stage_load: ") + e.what());
        return -1;
    }
}

double c4gpu_stage_load_ms(const c4gpu_stage *st) { return st->load_ms; }

void c4gpu_stage_destroy(c4gpu_stage *st) { delete st; g_retired.flush(); }

int c4gpu_batch_swap_stage(c4gpu_batch *b, c4gpu_stage *st) {
    if (!st->loaded) { c4h::set_error("c4gpu_batch_swap_stage: the stage holds no loaded batch"); return -1; }
    if (memcmp(&b->model, &st->model, sizeof(c4gpu_model)) || memcmp(&b->params, &st->params, sizeof(c4gpu_params))) {
        c4h::set_error("c4gpu_batch_swap_stage: batch and stage were made for different models / parameters");
        return -1;
    }
    b->clear_loop();
    for (auto &a : b->alignments) c4gpu_alignment_clear(&a);
    b->alignments.clear(); b->scores.clear(); b->regions.clear(); b->pair_thresholds.clear();
    b->seqs.swap_with(st->seqs);
    b->annotation_applied = false;                   // (a stage's codes are the residues': a load wrote them)
    st->loaded = false;
    return 0;
}

int c4gpu_batch_run(c4gpu_batch *b, int what, int dpmemory_mb, c4gpu_score threshold) {
    try {
        if (hipSetDevice(b->ctx->device) != hipSuccess) return -1;
        const int n = b->seqs.n_pairs;
        if (what == 0 || what == 1) {
            std::vector<JobOut> outs;
            if (score_pass(b->eng, b->seqs, what == 0 ? MODE_SCORE : MODE_REGION, outs)) return -1;
            b->scores.resize(n); b->regions.resize(n);
            for (int i = 0; i < n; i++) {
                const DevResult &r = outs[i].res;
                b->scores[i] = r.score;
                b->regions[i] = c4gpu_region{r.qs, r.ts, r.qe - r.qs, r.te - r.ts};
            }
            return 0;
        }
        for (auto &a : b->alignments) c4gpu_alignment_clear(&a);
        b->alignments.assign(n, c4gpu_alignment{});
        b->clear_loop();
        if (!b->side && !b->eng.annotated && lanes_wanted(b->seqs, nullptr, false)) {
            b->side.reset(new SideLane);
            if (b->side->init(b->ctx, &b->model, &b->params)) { b->side.reset(); return -1; }
        }
        if (find_path_lanes(b->eng, b->side.get(), b->seqs, dpmemory_mb, threshold, b->alignments.data(), nullptr,
                            b->pair_thresholds.empty() ? nullptr : &b->pair_thresholds)) return -1;
        b->scores.resize(n); b->regions.resize(n);
        for (int i = 0; i < n; i++) { b->scores[i] = b->alignments[i].score; b->regions[i] = b->alignments[i].region; }
        return 0;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_batch_run: ") + e.what());
        return -1;
    }
}

int c4gpu_batch_run_regions(c4gpu_batch *b, const c4gpu_region *regions, const uint8_t *active, int dpmemory_mb,
                            c4gpu_score threshold) {
    try {
        if (hipSetDevice(b->ctx->device) != hipSuccess) return -1;
        const int n = b->seqs.n_pairs;
        for (int i = 0; i < n; i++) {
            if (active && !active[i]) continue;
            const c4gpu_region &r = regions[i];
            if (r.query_start < 0 || r.target_start < 0 || r.query_length < 0 || r.target_length < 0 ||
                r.query_start + r.query_length > b->seqs.qlen[i] || r.target_start + r.target_length > b->seqs.tlen[i]) {
                c4h::set_error("c4gpu_batch_run_regions: a region lies outside its pair");
                return -1;
            }
        }
        for (auto &a : b->alignments) c4gpu_alignment_clear(&a);
        b->alignments.assign(n, c4gpu_alignment{});
        b->clear_loop();
        if (!b->side && !b->eng.annotated && lanes_wanted(b->seqs, active, false)) {
            b->side.reset(new SideLane);
            if (b->side->init(b->ctx, &b->model, &b->params)) { b->side.reset(); return -1; }
        }
        if (find_path_lanes(b->eng, b->side.get(), b->seqs, dpmemory_mb, threshold, b->alignments.data(), active, nullptr, regions))
            return -1;
        b->scores.resize(n); b->regions.resize(n);
        for (int i = 0; i < n; i++) { b->scores[i] = b->alignments[i].score; b->regions[i] = b->alignments[i].region; }
        return 0;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_batch_run_regions: ") + e.what());
        return -1;
    }
}

int c4gpu_batch_set_annotation(c4gpu_batch *b, const int32_t *cds_start, const int32_t *cds_length) {
    try {
        if (hipSetDevice(b->ctx->device) != hipSuccess) return -1;
        const int n = b->seqs.n_pairs;
        bool any = false;
        std::vector<int> cds(3 * (size_t)std::max(n, 1), 0);
        for (int i = 0; i < n; i++) {
            const int len = (cds_start && cds_length) ? cds_length[i] : 0;
            cds[3 * i] = len > 0 ? cds_start[i] : 0; cds[3 * i + 1] = len > 0 ? len : 0; cds[3 * i + 2] = b->seqs.qlen[i];
            any |= len > 0;
        }
        for (int c = 0; any && c < b->model.n_calcs; c++)
            if (b->model.calcs[c].kind == C4GPU_CALC_MATCH_CODON) {
                // Match_3_3_split_score_func vetoes by the frame of the annotated CDS (match.c:513-519): not built
                c4h::set_error(std::string("c4gpu_batch_set_annotation: model [") + b->model.name +
                               "] matches translated codons; the frame-dependent annotation veto of the 3:3 match is not supported");
                return -1;
            }
        // the veto belongs to the 1:1 DNA match calc alone (Engine::init_host decides it the same way): a model without one
        // keeps its codes, its parameter block, its kernels and its second lane
        bool dna_match = false, protein = false;
        for (int c = 0; c < b->model.n_calcs; c++) {
            const int kind = b->model.calcs[c].kind;
            dna_match |= kind == C4GPU_CALC_MATCH_DNA;
            protein |= kind == C4GPU_CALC_MATCH_PROTEIN || kind == C4GPU_CALC_MATCH_P2D || kind == C4GPU_CALC_MATCH_CODON;
        }
        if (!dna_match || protein) return 0;
        // pairs that were handed the same query buffer read the same codes (ResidentSeqs::build: one qoff): one annotation
        // between them, "none" being a value too; refused before anything is touched.  An empty query holds no codes and does
        // not advance the offsets (its qoff is the next query's): it shares nothing and its annotation reaches nothing
        {
            std::map<long long, int> first;
            for (int i = 0; i < n; i++) {
                if (b->seqs.qlen[i] == 0) continue;
                auto it = first.emplace(b->seqs.qoff[i], i).first;
                const int j = it->second;
                if (cds[3 * i] != cds[3 * j] || cds[3 * i + 1] != cds[3 * j + 1]) {
                    c4h::set_error("c4gpu_batch_set_annotation: pairs " + std::to_string(j) + " and " + std::to_string(i) +
                                   " share a query buffer and carry different annotations (give each its own copy of the query)");
                    return -1;
                }
            }
        }
        if (any != b->eng.annotated) {
            // the engine's guards and its parameter block follow (Engine::init_host): the veto row armed, the kernels that keep
            // every validity mask, no packed pass, one launch lane (the second lane's engine is built from the same
            // model and parameters and knows nothing of the annotation)
            b->eng.annotated = any;
            if (b->eng.init(b->ctx, &b->model, &b->params)) return -1;
            b->extra.clear();
            b->side.reset();
        }
        if (b->annotation_applied) {
            // the codes as the residues give them (an annotation that is taken away or replaced)
            hipLaunchKernelGGL(encode_kernel, dim3(1024), dim3(256), 0, b->ctx->stream, b->seqs.qraw.p, b->seqs.qcode.p,
                               (long long)(b->seqs.total_q + 64), b->seqs.tables.p, b->seqs.bad.p);
            HIP_OK(hipGetLastError());
            b->annotation_applied = false;
        }
        if (any) {
            DevBuf<int> d_cds;
            if (d_cds.upload(cds.data(), cds.size(), b->ctx->stream)) return -1;
            hipLaunchKernelGGL(annotate_qcode_kernel, dim3(n), dim3(64), 0, b->ctx->stream, b->seqs.qcode.p, b->seqs.dev.qoff,
                               d_cds.p, n);
            HIP_OK(hipGetLastError());
            b->annotation_applied = true;
        }
        HIP_OK(c4_stream_sync(b->ctx->stream));
        return 0;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_batch_set_annotation: ") + e.what());
        return -1;
    }
}

int c4gpu_batch_set_thresholds(c4gpu_batch *b, const c4gpu_score *per_pair) {
    if (!per_pair) { b->pair_thresholds.clear(); return 0; }
    b->pair_thresholds.assign(per_pair, per_pair + b->seqs.n_pairs);
    return 0;
}

// GAM_Result_exhaustive_create's do/while (gam.c:1158-1172) for the whole batch: block what the previous
// round found (GAM_Result_add_alignment -> SubOpt_add_alignment, gam.c:673), then the next best paths.
int c4gpu_batch_next_paths(c4gpu_batch *b, int dpmemory_mb, c4gpu_score threshold) {
    try {
        if (hipSetDevice(b->ctx->device) != hipSuccess) return -1;
        const int n = b->seqs.n_pairs;
        if ((int)b->alignments.size() != n) { c4h::set_error("c4gpu_batch_next_paths needs a c4gpu_batch_run(b, 2, ...) first"); return -1; }
        if (b->subopts.empty()) {
            b->subopts.resize(n);
            for (int i = 0; i < n; i++) b->subopts[i] = c4gpu_subopt_create(b->seqs.qlen[i], b->seqs.tlen[i]);
            b->in_loop.assign(n, 1);
        }
        std::vector<const c4gpu_subopt *> subs(n);
        int still = 0;
        for (int i = 0; i < n; i++) {
            if (b->in_loop[i] && b->alignments[i].valid) {
                if (c4gpu_subopt_add_alignment(b->subopts[i], &b->model, &b->alignments[i])) return -1;
                still++;
            } else {
                b->in_loop[i] = 0;
            }
            subs[i] = b->subopts[i];
        }
        for (auto &a : b->alignments) c4gpu_alignment_clear(&a);
        if (!still) return 0;
        if (find_path_batch(b->eng, b->seqs, dpmemory_mb, threshold, b->alignments.data(), &subs, b->in_loop.data(),
                            b->pair_thresholds.empty() ? nullptr : &b->pair_thresholds)) return -1;
        int found = 0;
        for (int i = 0; i < n; i++) {
            found += b->alignments[i].valid ? 1 : 0;
            b->scores[i] = b->alignments[i].score; b->regions[i] = b->alignments[i].region;
        }
        return found;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_batch_next_paths: ") + e.what());
        return -1;
    }
}

int c4gpu_batch_scores(c4gpu_batch *b, c4gpu_score *scores, c4gpu_region *regions) {
    for (size_t i = 0; i < b->scores.size(); i++) {
        if (scores) scores[i] = b->scores[i];
        if (regions) regions[i] = b->regions[i];
    }
    return (int)b->scores.size();
}

int c4gpu_batch_alignment(c4gpu_batch *b, int32_t i, c4gpu_alignment *out) {
    if (i < 0 || i >= (int)b->alignments.size()) return -1;
    const c4gpu_alignment &a = b->alignments[i];
    *out = a;
    out->op_transition = out->op_length = nullptr;
    if (a.n_ops) {
        out->op_transition = (int32_t *)malloc(sizeof(int32_t) * a.n_ops);
        out->op_length = (int32_t *)malloc(sizeof(int32_t) * a.n_ops);
        memcpy(out->op_transition, a.op_transition, sizeof(int32_t) * a.n_ops);
        memcpy(out->op_length, a.op_length, sizeof(int32_t) * a.n_ops);
    }
    return 0;
}

// every alignment of the batch in one int32 stream: first a row of 7 ints per pair (valid, score, region (4), n_ops), then
// the (transition, length) pairs of all valid alignments in pair order; returns the ints needed (written only when they
// fit `cap`): what a rank ships to the rank that prints
int64_t c4gpu_batch_export(c4gpu_batch *b, int32_t *out, int64_t cap) {
    int64_t need = 7 * (int64_t)b->alignments.size();
    for (const c4gpu_alignment &a : b->alignments) need += a.valid ? 2 * (int64_t)a.n_ops : 0;
    if (!out || need > cap) return need;
    int64_t pos = 0, ops = 7 * (int64_t)b->alignments.size();
    for (const c4gpu_alignment &a : b->alignments) {
        out[pos++] = a.valid; out[pos++] = a.valid ? a.score : 0;
        out[pos++] = a.region.query_start; out[pos++] = a.region.target_start;
        out[pos++] = a.region.query_length; out[pos++] = a.region.target_length;
        out[pos++] = a.valid ? a.n_ops : 0;
        if (a.valid) for (int k = 0; k < a.n_ops; k++) { out[ops++] = a.op_transition[k]; out[ops++] = a.op_length[k]; }
    }
    return need;
}

int c4gpu_batch_kernel_stats(c4gpu_batch *b, int mode, int reset, double *ms, int64_t *launches, int64_t *cells) {
    c4gpu_ctx *ctx = b->ctx;
    if (mode < 0 || mode > 3) return -1;
    c4gpu_ctx *lanes[2] = {ctx, b->side ? &b->side->ctx : nullptr};        // a large batch runs on two lanes (find_path_lanes)
    if (ms) *ms = 0;
    if (launches) *launches = 0;
    if (cells) *cells = 0;
    for (c4gpu_ctx *c : lanes) {
        if (!c) continue;
        if (ms) *ms += c->kernel_ms[mode];
        if (launches) *launches += c->kernel_launches[mode];
        if (cells) *cells += c->kernel_cells[mode];
        if (reset) { c->kernel_ms[mode] = 0; c->kernel_launches[mode] = 0; c->kernel_cells[mode] = 0; }
        c->timing = true;
    }
    return 0;
}

}  // extern "C"

