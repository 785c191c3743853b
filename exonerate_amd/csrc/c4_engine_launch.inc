// c4_engine_launch.inc -- part of c4_engine.hip (one translation unit; included there, in this order): job lists and kernel launches: JobSpec / JobOut / SeedPlan, Engine (kernel choice per launch, scratch slabs, the launch itself).
// ---- launching a list of jobs ---------------------------------------------------------------------------------
struct JobSpec {                  // host description of one Viterbi call
    int pair;
    c4gpu_region region;
    int first_state = 0, final_state = 1, cp_count = 0;
    int root = 0;                        // the state the path's END is entered from, for the kernels that only compute that state's
                                         // component (Roots, c4_viterbi16_kernel.h); 0: not known
    int first_cell[CELL_MAX] = {0};
    bool dump_checkpoints = false;
    const c4gpu_subopt *sub = nullptr;   // sub-optimal blocking for this call (else the engine's per-pair table)
    const int32_t *span_in = nullptr;    // span models: start cells (host), END cells (host, updated in place)
    int32_t *span_out = nullptr;
};
typedef std::vector<std::pair<int32_t, int32_t>> RegionPoints;   // (target, query) in region coordinates, ascending
// the runs of one path: the sub-alignments between checkpoints are a handful of runs each and there are
// hundreds of thousands of them per batch, so short lists live inline (no allocation per job)
struct RunList {
    static constexpr int INLINE = 6;
    int n = 0;
    uint32_t small[INLINE];
    std::vector<uint32_t> big;
    const uint32_t *begin() const { return n <= INLINE ? small : big.data(); }
    const uint32_t *end() const { return begin() + n; }
    void assign_reversed(const uint32_t *first, int count) {
        n = count;
        uint32_t *dst = small;
        if (count > INLINE) { big.resize(count); dst = big.data(); }
        for (int k = 0; k < count; k++) dst[k] = first[count - 1 - k];
    }
};
struct JobOut {
    DevResult res;
    RunList runs;                 // PATH: (transition << 24 | length) runs, START -> END
    std::vector<DevVsa> vsa;      // CKPT: sub-alignments, last section first
    std::vector<int> checkpoints; // CKPT + dump_checkpoints
    bool packed = false;          // CKPT: the cells come from the packed 16-bit pass (final_cell_equiv)
};

// The windowed region pass (c4_viterbi_kernel.h, SEED): what a launch needs to know about the column dumps.
struct SeedPlan {
    int mode = 0;                  // 1: the score pass writes dumps; 2: the region windows start from them
    int kshift = 11;               // a dump every 1 << kshift columns
    bool fmt16 = false;            // the dumps are the packed score pass's 16-bit rows (Dump16), read by the packed windows
                                   // (c4_win16_kernel.h): set by the mode 1 run, handed on to the mode 2 run
    int seedw = 0, dc = 0;         // ints per dumped row, dumped columns per dump: of the kernel the mode 1 run took
    std::vector<long long> off;    // per spec: mode 1 (out) start of the job's dumps; mode 2 (in) the dump to start from, -1 = none
    std::vector<int> rows;         // per spec, mode 2: rows of a dumped column (Q + 1 of the score pass)
    // mode 2, windows chained on the device (DevJob::seed_base ..): per spec the pair's first dump, the dump the first
    // window starts from, its lattice column, the target_start of the score pass's rectangle; hops: windows per job
    std::vector<long long> base;
    std::vector<int> d, t0w, t0_base;
    int hops = 0;
};

// a splice model's PSSM with every row at its best column: the sum of the rows' largest entries (magnitudes with `absolute`);
// a row without a positive entry adds nothing
double splice_best_sum(const c4gpu_splice_model &sp, bool absolute) {
    double sum = 0;
    for (int r = 0; r < sp.model_length && r < C4GPU_SPLICE_MAX_LEN; r++) {
        double mx = 0;
        for (int c = 0; c < 5; c++) mx = std::max(mx, absolute ? std::fabs((double)sp.data[r][c]) : (double)sp.data[r][c]);
        sum += mx;
    }
    return sum;
}

// ... and at its worst: the sum of the rows' smallest entries; a row without a negative entry adds nothing (the window of a
// position near an end of the sequence is clipped: any run of rows can be missing)
double splice_worst_sum(const c4gpu_splice_model &sp) {
    double sum = 0;
    for (int r = 0; r < sp.model_length && r < C4GPU_SPLICE_MAX_LEN; r++) {
        double mn = 0;
        for (int c = 0; c < 5; c++) mn = std::min(mn, (double)sp.data[r][c]);
        sum += mn;
    }
    return sum;
}

struct Engine {
    c4gpu_ctx *ctx;
    const c4gpu_model *model;
    int family;
    bool local;
    // The local-scope score / region kernels drop the row-0 validity mask (c4_viterbi_kernel.h, eval_cell):
    // a phantom candidate there is -987654321 plus one or two calc values and must stay far below every
    // candidate the reference has.  True while the calc magnitudes are small against 987654321; checked
    // here, and parameters outside that range get the general kernels (all masks kept) instead.
    bool local_exact = true;
    bool pk16_params_ok = false;         // see init: the parameters allow the packed 16-bit score pass
    // ... and its biased (staged) forms: no negative addend between PK16_ADDEND_MAX and "clamps to -32 768" (c4_pk16_bias.h)
    bool pk16_bias_ok = false;
    // largest magnitude one transition can add (calc constants, substitution scores, a splice model's best column sum):
    // what the continuation kernels without the row-0 mask need to stay exact (cont_free_ok)
    double calc_bound = 0;
    int pk16_match_max = 1, pk16_max_intron = 0;
    // what ONE intron can add to a path (best 5' sum + best 3' sum + the opening constant; 0 when that is negative, as with
    // the default parameters: 13 + 16 - 30) and the fewest target columns it takes: a path gains at most
    // (Q + 1) x pk16_match_max + (T / pk16_intron_cols + 1) x pk16_intron_gain (pk16_fits)
    int pk16_intron_gain = 0, pk16_intron_cols = 4;
    int loop_tr_host[16] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};     // KParams::loop_tr
    DevBuf<KParams> kparams;
    // reusable device buffers
    DevBuf<DevJob> d_jobs;
    DevBuf<DevResult> d_results;
    DevBuf<DevVsa> d_vsa;
    DevBuf<uint32_t> d_runs, d_runs_out;
    DevBuf<unsigned long long> d_runs_used;
    DevBuf<uint8_t> d_ops;
    DevBuf<int> d_bnd, d_ckpt, d_ckpt_dump, d_queue;
    DevBuf<uint32_t> d_tb;
    DevBuf<int> d_sub_t, d_sub_q, d_sub_colptr, d_span, d_seed, d_pairs;
    // fused_reduced_paths: checkpoint jobs, their results and sub-alignment lists, the sub-alignment jobs built from them
    DevBuf<DevJob> d_fjobs, d_fsub_jobs;
    DevBuf<DevResult> d_fres, d_fsub_res;
    DevBuf<DevVsa> d_fvsa;
    DevBuf<int> d_ffirst, d_fflags, d_fout;
    DevBuf<unsigned long long> d_fstats;
    DevBuf<FusePair> d_fpairs;
    std::vector<DevJob> hf_jobs;
    std::vector<DevResult> hf_res;
    std::vector<int> hf_first, hf_flags, hf_out;
    std::vector<FusePair> hf_pairs;
    // reusable host staging of run_impl (a sub-alignment launch lists ~10^5 jobs: fresh vectors of that size
    // are page-faulted in on every call)
    std::vector<int> h_order;
    std::vector<long long> h_key;
    std::vector<int> h_qlen;                // the jobs' query lengths, as the kernel choice reads them
    std::vector<DevJob> h_jobs;
    std::vector<DevResult> h_res;
    std::vector<uint32_t> h_runs;
    std::vector<DevVsa> h_vsa;
    std::vector<int> h_dump;
    std::vector<JobSpec> fp_specs;          // ... and of find_path_batch
    std::vector<JobSpec> fp_sub_specs;      // its sub-alignment launch (every entry rewritten; only resized when the count changes)
    std::vector<JobOut> fp_outs;
    // per-pair SubOpt of the Optimal_find_path in progress (NULL entries / NULL table: nothing blocked)
    const std::vector<const c4gpu_subopt *> *pair_sub = nullptr;

    // c4gpu_batch_set_annotation: some query of the batch has a CDS annotation (init_host then arms the veto row and takes the
    // guarded kernels; init must run again after a change)
    bool annotated = false;
    int init(c4gpu_ctx *c, const c4gpu_model *m, const c4gpu_params *params) {
        KParams kp;
        if (init_host(c, m, params, kp)) return -1;
        return kparams.upload(&kp, 1, ctx->stream);
    }
    // everything init decides on the host (family, guards of the shortcuts and of the packed passes): no device call
    int init_host(c4gpu_ctx *c, const c4gpu_model *m, const c4gpu_params *params, KParams &kp) {
        ctx = c; model = m;
        family = model_family(*m);
        if (family < 0) {
            c4h::set_error(std::string("model [") + m->name + "] is not one of the device-accelerated families");
            return -1;
        }
        local = m->start_scope == C4GPU_SCOPE_ANYWHERE && m->end_scope == C4GPU_SCOPE_ANYWHERE;
        memset(&kp, 0, sizeof kp);
        for (int i = 0; i < 16; i++) loop_tr_host[i] = -1;
        for (int i = 0; i < m->n_calcs; i++) kp.calc_value[i] = m->calcs[i].value;
        kp.min_intron = params->min_intron; kp.max_intron = params->max_intron;
        if (params->max_intron < params->min_intron) {
            // the reference would reject every intron (length < min or > max is always true); the device
            // test folds both comparisons into one and needs a non-negative span for that
            kp.min_intron = kp.max_intron = 0x7fffffff;     // span 0 at a length no intron has: always rejected
        }
        kp.start_scope = m->start_scope; kp.end_scope = m->end_scope;
        bool protein = false;
        for (int i = 0; i < m->n_calcs; i++)
            if (m->calcs[i].kind == C4GPU_CALC_MATCH_PROTEIN || m->calcs[i].kind == C4GPU_CALC_MATCH_P2D ||
                m->calcs[i].kind == C4GPU_CALC_MATCH_CODON) protein = true;
        memcpy(kp.submat, protein ? &params->protein_submat[0][0] : &params->dna_submat[0][0], sizeof(int) * 24 * 24);
        // --annotation (match.c:276-281): a DNA query position inside its CDS may not take part in a 1:1 DNA match: such
        // positions carry row code 24 (annotate_qcode_kernel), whose row scores MATCH_IMPOSSIBLY_LOW_SCORE against everything
        bool dna_match = false;
        for (int i = 0; i < m->n_calcs; i++) dna_match |= m->calcs[i].kind == C4GPU_CALC_MATCH_DNA;
        const bool veto = annotated && dna_match && !protein;
        for (int c = 0; c < 24; c++) kp.submat[24 * 24 + c] = veto ? C4GPU_IMPOSSIBLY_LOW_SCORE : 0;
        {
            // largest magnitude one calc can contribute (the -987654321 sentinel of --forcegtag aside: it is
            // the same number in the reference)
            double pmax = 0;
            for (int i = 0; i < m->n_calcs; i++) pmax = std::max(pmax, std::fabs((double)m->calcs[i].value));
            for (int i = 0; i < 24 * 24; i++) pmax = std::max(pmax, std::fabs((double)kp.submat[i]));
            double smax = 0;
            if (family_has_splice(family))
                for (int k = 0; k < 4; k++) smax = std::max(smax, splice_best_sum(params->splice[k], true) + 1.0);
            // a real candidate is at least -(states x largest calc); a phantom one at most LOW + 3 calcs
            local_exact = (pmax + smax) * (m->n_states + 4) < 4.0e8;
            calc_bound = pmax + smax;
            // the packed 16-bit score pass (c4_viterbi16_kernel.h): every constant far inside 16 bits, a usual intron window
            double mmax = 0;
            for (int i = 0; i < 24 * 24; i++) mmax = std::max(mmax, (double)kp.submat[i]);
            pk16_match_max = (int)std::max(1.0, mmax);
            pk16_params_ok = pmax <= (double)PK16_SCORE_MAX && smax <= (double)PK16_SCORE_MAX && params->min_intron >= 0 && params->min_intron <= 30000 &&
                             params->max_intron >= params->min_intron;
            pk16_max_intron = params->max_intron;
            pk16_bias_ok = false;
            if (veto) {
                // a match score of -987654321 is no "small calc": the kernels that keep every validity mask and the 32-bit
                // passes serve such batches (what parameters of that magnitude get: *_hugegap sets)
                local_exact = false;
                pk16_params_ok = false;
                calc_bound = std::max(calc_bound, 987654321.0);
            }
            if (family_has_splice(family)) {
                // largest value a site of each kind can score: every PSSM row at its best, rounded as the predictor rounds
                int best[4];
                for (int k = 0; k < 4; k++) best[k] = (int)std::floor(splice_best_sum(params->splice[k], false) + 0.5) + 1;
                // an intron enters its state through a pre-splice transition and leaves it through a post-splice transition OF THE
                // SAME STATE (est2genome: the forward strand's intron state and the reverse strand's are two states that share
                // nothing): the most one intron can add is the best such pairing per state, not the best pre-site of one strand
                // with the best post-site of the other (rounds 3-4: that bound put 2 x T / 30 on top of every query; per state
                // it is 1, and 1 kb x 100 kb queries of up to ~2 500 nt fit where ~1 865 did)
                long long gain = -0x40000000LL;
                for (int st = 0; st < m->n_states; st++) {
                    long long pre = -0x40000000LL, post = -0x40000000LL;
                    for (int k = 0; k < m->n_transitions; k++) {
                        const c4gpu_transition &t = m->transitions[k];
                        if (t.calc < 0) continue;
                        const c4gpu_calc &cc = m->calcs[t.calc];
                        const int prm = cc.param & 3;
                        if (cc.kind == C4GPU_CALC_SPLICE_PRE && t.output == st) pre = std::max<long long>(pre, (long long)cc.value + best[prm]);
                        if (cc.kind == C4GPU_CALC_SPLICE_POST && t.input == st) post = std::max<long long>(post, (long long)cc.value + best[prm]);
                    }
                    if (pre > -0x40000000LL && post > -0x40000000LL) gain = std::max(gain, pre + post);
                }
                // the biased forms: every site at its worst, rounded as the predictor rounds (one more for the float sums), with
                // the calc constant of a pre-splice transition folded in as ss16_kernel / SpliceFold fold it (--forcegtag's
                // -987 654 321 is written in a sum's place and clamps to exactly -32 768, which those forms carry)
                long long site_worst[4] = {0, 0, 0, 0}, post_best = 0;
                for (int i = 0; i < m->n_calcs; i++) {
                    const c4gpu_calc &cc = m->calcs[i];
                    const int prm = cc.param & 3;
                    const long long worst = (long long)std::floor(splice_worst_sum(params->splice[prm]) - 0.5) - 1;
                    if (cc.kind == C4GPU_CALC_SPLICE_PRE) site_worst[prm] = std::min(site_worst[prm], (long long)cc.value + worst);
                    if (cc.kind == C4GPU_CALC_SPLICE_POST) {
                        site_worst[prm] = std::min(site_worst[prm], worst);
                        post_best = std::max<long long>(post_best, best[prm]);
                    }
                }
                pk16_bias_ok = pk16_bias_fits(kp.submat, 24 * 24, kp.calc_value, m->n_calcs, site_worst, 4, post_best);
                pk16_intron_gain = (int)std::max<long long>(0, std::min<long long>(gain, 1 << 20));
                pk16_intron_cols = std::max(4, params->min_intron);
                // KParams::loop_tr (c4_viterbi_kernel.h, viterbi_kernel): a state s with a loop (0, 1) that adds nothing, entered
                // by pre-splice and left by post-splice transitions only, where leaving and coming back cannot pay: the best
                // 3' site + the best 5' site + the opening constant of s's own transitions is NEGATIVE (the sites at their best
                // as the predictor rounds them, splice.c:379-381 -- without the + 1 of slack the 16-bit guard above allows
                // itself, but with 0.001 for the float sums: 13 + 15 - 30 = -2 under the default parameters), and nothing
                // else that moves along the target without a query row adds anything (gaps cost).  Then every cell of a
                // one-row continuation from s takes the loop, whatever the order of the candidates.  C4GPU_LOOP_SHORTCUT=0: off.
                const bool loop_on = !(c4cfg::is(c4cfg::LOOP_SHORTCUT, 0));
                bool others_cost = true;
                for (int k = 0; k < m->n_transitions; k++) {
                    const c4gpu_transition &t = m->transitions[k];
                    if (t.advance_query != 0 || t.calc < 0) continue;
                    const c4gpu_calc &cc = m->calcs[t.calc];
                    if (cc.kind == C4GPU_CALC_SPLICE_PRE || cc.kind == C4GPU_CALC_SPLICE_POST) continue;
                    if (cc.kind != C4GPU_CALC_CONST || cc.value > 0) others_cost = false;
                }
                if (loop_on && family == FAM_EST2GENOME && others_cost && m->n_states <= 16) {
                    int tight[4];
                    for (int k = 0; k < 4; k++) tight[k] = (int)std::floor(splice_best_sum(params->splice[k], false) + 0.5 + 1e-3);
                    for (int st = 0; st < m->n_states; st++) {
                        long long pre = -0x40000000LL, post = -0x40000000LL;
                        int loop = -1;
                        bool clean = true;
                        for (int k = 0; k < m->n_transitions; k++) {
                            const c4gpu_transition &t = m->transitions[k];
                            const c4gpu_calc *cc = t.calc >= 0 ? &m->calcs[t.calc] : nullptr;
                            if (t.input == st && t.output == st) {
                                if (t.advance_query == 0 && t.advance_target == 1 && !cc && loop < 0) loop = k; else clean = false;
                            } else if (t.output == st) {
                                if (cc && cc->kind == C4GPU_CALC_SPLICE_PRE) pre = std::max<long long>(pre, (long long)cc->value + tight[cc->param & 3]);
                                else clean = false;
                            } else if (t.input == st) {
                                if (cc && cc->kind == C4GPU_CALC_SPLICE_POST) post = std::max<long long>(post, (long long)cc->value + tight[cc->param & 3]);
                                else clean = false;
                            }
                        }
                        loop_tr_host[st] = (clean && loop >= 0 && pre > -0x40000000LL && post > -0x40000000LL && pre + post < 0) ? loop : -1;
                    }
                }
            }
            if (c4cfg::is(c4cfg::LOCAL_EXACT, 0)) local_exact = false;   // test hook
        }
        for (int i = 0; i < 16; i++) kp.loop_tr[i] = loop_tr_host[i];
        if (c4cfg::has(c4cfg::TRACE) && family == FAM_EST2GENOME) {
            std::string which;
            for (int i = 0; i < 16; i++) if (loop_tr_host[i] >= 0) which += " " + std::to_string(i) + ":" + std::to_string(loop_tr_host[i]);
            fprintf(stderr, "c4gpu trace: one-row sections answered without a DP for states (state:loop transition)%s\n",
                    which.empty() ? " none" : which.c_str());
        }
        for (int c = 0; c < 4096; c++) {
            const uint8_t row = params->submat_index[params->aa[params->trans[c]]];
            kp.codon_row[c] = row < 24 ? row : 0;        // '-' (empty mask) never scores: such columns are rejected at upload
        }
        return 0;
    }

    // The continuation kernels compiled without the row-0 validity mask (c4_viterbi_kernel.h, eval_cell: CONT && LOCAL)
    // hold, in states the reference leaves unset, -987654321 plus at most one calc per cell of a path: exact while
    // that stays far below every real score of the job, i.e. (Q + T + 2) x the largest calc well under 987654321 / 2.
    // C4GPU_CONT_FREE=0 keeps the kernels with every mask.
    bool cont_free_ok(long long q_plus_t) const {
        if (c4cfg::is(c4cfg::CONT_FREE, 0)) return false;
        return (double)(q_plus_t + 2) * std::max(calc_bound, 1.0) < 4.0e8;
    }

    // The packed 16-bit passes (c4_viterbi16_kernel.h, c4_ckpt16_kernel.h) are exact while everything a path can gain stays
    // inside 16 000: the substitution scores of its query rows plus, where an intron's two sites can outweigh its opening
    // penalty (a small --intronpenalty), that net gain once per intron the target has room for; and the intron length test
    // must not be able to fail on the upper side (the packed length counter saturates).
    bool pk16_fits(int query_length, int target_length) const {
        const double gain = (double)(query_length + 1) * pk16_match_max +
                            (double)(target_length / pk16_intron_cols + 1) * pk16_intron_gain;
        return gain <= (double)PK16_SCORE_MAX && (!family_has_splice(family) || (long long)target_length + 4 <= (long long)pk16_max_intron);
    }
    // the four splice values of every target position as the packed passes add them (ss16_kernel): built once per batch,
    // finished before the lock is released (the other lane launches on another stream)
    int ensure_ss16(const ResidentSeqs &seqs) {
        if (!family_has_splice(family)) return 0;
        std::lock_guard<std::mutex> hold(seqs.ss16_lock);
        if (!seqs.ss16_built) {
            if (seqs.ss16.alloc((size_t)seqs.ss_len)) return -1;
            HIP_OK(pk16_build_splice(family, kparams.p, seqs.dev.ss, seqs.dev.ss_stride, seqs.ss_len, seqs.ss16.p, ctx->stream));
            HIP_OK(c4_stream_sync(ctx->stream));
            seqs.ss16_built = true;
        }
        return 0;
    }

    // Runs `specs` in `mode`; out[i] corresponds to specs[i].  Calls whose region holds blocked cells
    // (SubOpt_Index_create returns an index, subopt.c:250-266) go to the kernels compiled with blocking, the
    // others (it returns NULL) to the plain ones.
    int run(const ResidentSeqs &seqs, int mode, bool cont, const std::vector<JobSpec> &specs, std::vector<JobOut> &out,
            SeedPlan *seed = nullptr) {
        const int n = (int)specs.size();
        if (seed) return run_impl(seqs, mode, cont, specs, out, nullptr, seed);
        for (int i = 0; i < n; i++)
            if (specs[i].span_in || specs[i].span_out) return run_impl(seqs, mode, cont, specs, out, nullptr);
        std::vector<int> plain, blocked;
        std::vector<RegionPoints> pts;
        for (int i = 0; i < n; i++) {
            const c4gpu_subopt *so = specs[i].sub ? specs[i].sub : (pair_sub ? (*pair_sub)[specs[i].pair] : nullptr);
            RegionPoints rp;
            if (so && !so->points.empty()) c4h::subopt_region_points(so, specs[i].region, rp);
            if (rp.empty()) plain.push_back(i);
            else { blocked.push_back(i); pts.push_back(std::move(rp)); }
        }
        if (blocked.empty()) return run_impl(seqs, mode, cont, specs, out, nullptr);
        // a handful of calls without blocked cells would occupy a corner of the device for as long as a full
        // launch: they ride along in the blocking kernels with empty lists
        if (plain.size() * 4 < blocked.size()) {
            std::vector<RegionPoints> all(n);
            for (size_t x = 0; x < blocked.size(); x++) all[blocked[x]] = std::move(pts[x]);
            return run_impl(seqs, mode, cont, specs, out, &all);
        }
        out.assign(n, JobOut());
        std::vector<JobSpec> part;
        std::vector<JobOut> part_out;
        for (int i : plain) part.push_back(specs[i]);
        if (run_impl(seqs, mode, cont, part, part_out, nullptr)) return -1;
        for (size_t x = 0; x < plain.size(); x++) out[plain[x]] = std::move(part_out[x]);
        part.clear();
        for (int i : blocked) part.push_back(specs[i]);
        if (run_impl(seqs, mode, cont, part, part_out, &pts)) return -1;
        for (size_t x = 0; x < blocked.size(); x++) out[blocked[x]] = std::move(part_out[x]);
        return 0;
    }

    // the trace of one run_impl: a line per stage, the total when it ends
    struct RunTrace {
        bool on; std::chrono::steady_clock::time_point t0; int mode, n;
        double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
        void lap(const char *what) const { if (on) fprintf(stderr, "c4gpu trace:   %-18s at %.3f ms\n", what, ms()); }
        ~RunTrace() { if (on) fprintf(stderr, "c4gpu trace: run mode %d jobs %d host+device %.3f ms\n", mode, n, ms()); }
    };
    // what plan_jobs lays out for a launch (beside h_order and h_jobs): totals of the per-job buffers, the largest per-workgroup
    // scratch items, the blocked cells and the pairs of the two-jobs-per-lane kernels, the grid
    struct LaunchPlan {
        long long ops_total = 0, vsa_total = 0, dump_total = 0, max_T = 0, max_tb = 0, max_ckpt = 0, total_cells = 0;
        long long max_runs = 0, sub_cols = 0, span_total = 0, seed_total = 0;
        std::vector<int> sub_t, sub_q, pair_list;
        long long grid = 0, carry_T = 0, bnd_per_wave = 0;
    };
    static int nbits(int v) { int b = 0; while ((1LL << b) <= v) b++; return b; }

    int run_impl(const ResidentSeqs &seqs, int mode, bool cont, const std::vector<JobSpec> &specs,
                 std::vector<JobOut> &out, const std::vector<RegionPoints> *pts, SeedPlan *seed = nullptr) {
        const RunTrace tr{c4cfg::has(c4cfg::TRACE), std::chrono::steady_clock::now(), mode, (int)specs.size()};
        const int n = (int)specs.size();
        // every field of entries [0, n) is rewritten after the launch; a vector that is reused for launches of very
        // different sizes (4 096 checkpoint jobs, then 778 443 sub-alignments, every step) is never shrunk: building
        // and tearing down its tail was the largest host item of such a step
        if ((int)out.size() < n) out.resize(n);
        if (!n) return 0;
        // -- the facts of the launch, and the kernel that serves it (c4_kernel_choice.h); the switches are read on every call
        // so that a test can flip one
        const Switches sw = Switches::from_config();
        LaunchFacts f;
        f.family = family; f.mode = mode; f.cont = cont; f.n = n; f.blocked = pts != nullptr;
        f.local = local; f.local_exact = local_exact;
        // packed region-start slot: (query_start << tshift) | target_start must fit 31 bits for every job
        f.starts_pack = mode == MODE_REGION;
        for (int i = 0; i < n && f.starts_pack; i++)
            f.starts_pack = nbits(specs[i].region.query_length) + nbits(specs[i].region.target_length) <= 31;
        for (int i = 0; i < n; i++) {
            const int sp = specs[i].span_in ? 1 : (specs[i].span_out ? 2 : 0);
            if (i && sp != f.span) { c4h::set_error("jobs with and without span matrices in one call"); return -1; }
            f.span = sp;
        }
        const int span = f.span;
        if (cont && (mode == MODE_PATH || mode == MODE_CKPT) && !pts && !span) {
            long long worst = 0;
            bool cells_leave = false;             // checkpoint cells handed to the caller must be the reference's in every state
            for (int i = 0; i < n; i++) {
                worst = std::max(worst, (long long)specs[i].region.query_length + specs[i].region.target_length);
                cells_leave |= specs[i].dump_checkpoints;
            }
            f.cont_free = !cells_leave && cont_free_ok(worst);
        }
        if (seed) { f.seed_mode = seed->mode; f.kshift = seed->kshift; f.fmt16 = seed->fmt16; }
        f.pk16_params_ok = pk16_params_ok;
        f.pk16_bias_unfit = !pk16_bias_ok;
        f.pk16_all_fit = f.seed_mode == 1;
        for (int i = 0; i < n && f.pk16_all_fit; i++) f.pk16_all_fit = pk16_fits(specs[i].region.query_length, specs[i].region.target_length);
        f.tdense_n = seqs.tdense_n; f.ss16_built = seqs.ss16_built;
        f.cu_count = ctx->prop.multiProcessorCount;
        if (!cont) {
            h_qlen.resize(n);
            for (int i = 0; i < n; i++) h_qlen[i] = specs[i].region.query_length;
            f.query_length = h_qlen.data(); f.n_lengths = n;
        }
        const KernelChoice choice = choose_kernel(f, sw);
        if (choice.error) { c4h::set_error(choice.error); return -1; }
        const KernelInfo *ki = choice.ki;
        if (choice.needs_ss16 && ensure_ss16(seqs)) return -1;
        if (seed) {
            seed->fmt16 = choice.fmt16;
            if (seed->mode == 1) { seed->seedw = ki->seedw; seed->dc = ki->max_at; }
            if (tr.on) fprintf(stderr, "c4gpu trace:   seeded pass %d with kernel %s\n", seed->mode, ki->name);
        }
        const uint8_t *staged_codes = choice.staged_codes ? seqs.tdense.p : nullptr;     // the staged packed score pass's residue-code table
        LaunchPlan lp;
        if (plan_jobs(specs, mode, ki, pts, span, seed, tr, lp)) return -1;
        if (launch_jobs(seqs, mode, ki, specs, pts, span, seed, staged_codes, tr, lp)) return -1;
        tr.lap("runs downloaded");
        return unpack(mode, ki, n, out);
    }

    // The launch's jobs in the order the device takes them (h_order, h_jobs), their offsets into the launch's buffers and the
    // sizes of those, the grid.
    int plan_jobs(const std::vector<JobSpec> &specs, int mode, const KernelInfo *ki, const std::vector<RegionPoints> *pts, int span,
                  SeedPlan *seed, const RunTrace &tr, LaunchPlan &lp) {
        const int n = (int)specs.size();
        const int span_cs = 1 + model->total_shadow_designations;
        // longest first (persistent waves pull from the queue head)
        std::vector<int> &order = h_order;
        order.resize(n);
        std::iota(order.begin(), order.end(), 0);
        auto cells = [&](int i) { return (long long)(specs[i].region.query_length + 1) * (specs[i].region.target_length + 1); };
        {
            // ... unless the launch is tens of thousands of small jobs (the sub-alignments between checkpoints):
            // any order balances those, and sorting them is then the largest item on the host
            std::vector<long long> &key = h_key;
            key.resize(n);
            long long biggest = 0;
            for (int i = 0; i < n; i++) { key[i] = cells(i); biggest = std::max(biggest, key[i]); }
            if (ki->pairs)         // two jobs per lane, paired by the host: jobs of one root together, each group longest first
                std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                    return specs[a].root != specs[b].root ? specs[a].root < specs[b].root : key[a] > key[b];
                });
            else if (!(n > 32768 && biggest < (1 << 20)))
                std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] > key[b]; });
        }
        std::vector<DevJob> &jobs = h_jobs;
        jobs.resize(n);
        if (seed && seed->mode == 1) seed->off.assign(n, -1);
        // the fields that do not depend on the jobs before it ...
        parallel_for(n, 32768, [&](long long first, long long last) {
            for (long long x = first; x < last; x++) {
                const JobSpec &s = specs[order[x]];
                DevJob &j = jobs[x];
                memset(&j, 0, sizeof j);
                j.seed_off = -1;
                if (seed) j.seed_kshift = seed->kshift;
                j.pair = s.pair; j.q0 = s.region.query_start; j.t0 = s.region.target_start;
                j.Q = s.region.query_length; j.T = s.region.target_length;
                j.first_state = s.first_state; j.final_state = s.final_state; j.cp_count = s.cp_count;
                j.root = s.root;
                j.tshift = nbits(j.T);
                memcpy(j.first_cell, s.first_cell, sizeof j.first_cell);
                j.ckpt_off = -1;
            }
        });
        // ... and the running offsets into the launch's buffers
        for (int x = 0; x < n; x++) {
            const JobSpec &s = specs[order[x]];
            DevJob &j = jobs[x];
            if (span) {
                j.span_off = lp.span_total;
                lp.span_total += (long long)(s.region.query_length + 1) * (s.region.target_length + 1) * span_cs;
            }
            if (pts) {
                const RegionPoints &rp = (*pts)[order[x]];
                j.sub_off = lp.sub_cols; j.sub_pt_off = (int)lp.sub_t.size(); j.sub_pt_n = (int)rp.size();
                lp.sub_cols += s.region.target_length + 2;
                for (const auto &p : rp) { lp.sub_t.push_back(p.first); lp.sub_q.push_back(p.second); }
            }
            if (seed) {
                if (seed->mode == 1) {            // dumps d = 1 .. T >> kshift, two columns of Q + 1 rows each
                    j.seed_off = lp.seed_total; j.seed_rows = s.region.query_length + 1;
                    seed->off[order[x]] = lp.seed_total;
                    lp.seed_total += (long long)(s.region.target_length >> seed->kshift) * ki->max_at * (s.region.query_length + 1) *
                                  ki->seedw;
                } else {
                    j.seed_off = seed->off[order[x]]; j.seed_rows = seed->rows[order[x]];
                    if (seed->hops) {
                        j.seed_base = seed->base[order[x]]; j.win_d = seed->d[order[x]]; j.win_t0w = seed->t0w[order[x]];
                        j.win_t0_base = seed->t0_base[order[x]]; j.win_hops = seed->hops;
                    }
                }
            }
            j.ops_off = lp.ops_total; j.ops_cap = 0; j.vsa_off = (int)lp.vsa_total;
            lp.total_cells += (long long)(j.Q + 1) * (j.T + 1);
            lp.max_T = std::max<long long>(lp.max_T, j.T);
            if (mode == MODE_PATH) {
                const long long strips = (j.Q + 1 + 64 * ki->R - 1) / (64 * ki->R);
                j.ops_cap = 3 * (j.Q + j.T) + 16;
                lp.max_runs = std::max<long long>(lp.max_runs, j.ops_cap);
                lp.ops_total += j.ops_cap;
                lp.max_tb = std::max(lp.max_tb, strips * (long long)(j.T + 64) * 64 * ki->R);
            }
            if (mode == MODE_CKPT) {
                const long long ck = (long long)j.cp_count * ki->max_at * (j.Q + 1) * ki->n_states * ki->cs;
                lp.max_ckpt = std::max(lp.max_ckpt, ck);
                lp.vsa_total += j.cp_count + 1;
                if (s.dump_checkpoints) { j.ckpt_off = lp.dump_total; lp.dump_total += ck; }
            }
        }
        // windows chained on the device: a later window of a job spans one dump interval plus the dumped columns, which can be
        // more than every FIRST window of the launch: the strip carry rows are laid out for the longest window any hop can have
        if (seed && seed->mode == 2 && seed->hops)
            lp.max_T = std::max<long long>(lp.max_T, (1LL << seed->kshift) + 2LL * ki->max_at);
        tr.lap("jobs built");
        // persistent grid: as many waves as the device keeps resident, bounded by the scratch it implies
        int blocks_per_cu = 0;
        HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, ki->func, 64 * ki->waves, 0));
        if (blocks_per_cu < 1) blocks_per_cu = 1;
        if (tr.on) fprintf(stderr, "c4gpu trace:   kernel %s: %d workgroups per CU\n", ki->name, blocks_per_cu);
        // the kernels that run two jobs per lane in pairs the host lists: neighbours of the same root
        if (ki->pairs)
            for (int x = 0; x < n;) {
                const bool two = x + 1 < n && jobs[x + 1].root == jobs[x].root;
                lp.pair_list.push_back(x); lp.pair_list.push_back(two ? x + 1 : -1);
                x += two ? 2 : 1;
            }
        lp.grid = std::min<long long>(ki->pairs ? (long long)lp.pair_list.size() / 2 : n, (long long)blocks_per_cu * ctx->prop.multiProcessorCount);
        // strip carry rows in HBM are only needed when a job has more strips than one workgroup holds at once
        // (one for the single-wave kernels, `waves` for the cooperating ones)
        for (int x = 0; x < n; x++)
            if ((jobs[x].Q + 1 + 64 * ki->R - 1) / (64 * ki->R) > (ki->hbm_carry ? 1 : ki->waves)) lp.carry_T = lp.max_T;
        // per workgroup: one "empty" column (what the first strip reads as its row above) + two carry rows
        lp.bnd_per_wave = (2 * ((lp.carry_T ? lp.carry_T : 0) + 1) + 1) * (long long)std::max(ki->bnd, 1);
        const long long bytes_per_wave = lp.bnd_per_wave * 4 + lp.max_tb * 4 + lp.max_ckpt * 4 + lp.max_runs * 4;
        const long long budget = (long long)(ctx->prop.totalGlobalMem / 4);
        if (bytes_per_wave * lp.grid > budget) lp.grid = std::max<long long>(1, budget / std::max<long long>(1, bytes_per_wave));
        return 0;
    }

    // Uploads what plan_jobs laid out, launches, downloads the results; a launch whose traceback runs overflow the compact run
    // array is repeated once with the worst case.  Leaves the results in h_res, h_runs, h_vsa, h_dump.
    int launch_jobs(const ResidentSeqs &seqs, int mode, const KernelInfo *ki, const std::vector<JobSpec> &specs,
                    const std::vector<RegionPoints> *pts, int span, SeedPlan *seed, const uint8_t *staged_codes, const RunTrace &tr,
                    LaunchPlan &lp) {
        const int n = (int)specs.size();
        const int span_cs = 1 + model->total_shadow_designations;
        const std::vector<int> &order = h_order;
        const std::vector<DevJob> &jobs = h_jobs;
        hipStream_t s = ctx->stream;
        // compact run array: paths are mostly long runs, so a fraction of the worst case is plenty; a
        // launch that overflows it is repeated with the worst case
        long long runs_capacity = std::min<long long>(lp.ops_total, std::max<long long>(1 << 20, (long long)n * 256));
        std::vector<DevResult> &res = h_res;
        res.resize(n);
        std::vector<uint32_t> &runs = h_runs;
        runs.clear();
        std::vector<DevVsa> &vsa = h_vsa;         // kept between launches: fresh vectors of this size are zeroed and
        std::vector<int> &dump = h_dump;          // page-faulted in on every call (50 MB for a C2-shaped batch)
        vsa.resize(lp.vsa_total);
        dump.resize(lp.dump_total);
        for (int attempt = 0; attempt < 2; attempt++) {
            int zero = 0;
            unsigned long long zero64 = 0;
            if (d_jobs.upload(jobs.data(), n, s) || d_results.alloc(n) || d_queue.upload(&zero, 1, s) ||
                d_runs_used.upload(&zero64, 1, s) || d_bnd.alloc(lp.bnd_per_wave * lp.grid) || d_vsa.alloc(lp.vsa_total) ||
                d_runs.alloc(lp.max_runs * lp.grid) || d_runs_out.alloc(runs_capacity) ||
                d_tb.alloc(lp.max_tb * lp.grid) || d_ckpt.alloc(lp.max_ckpt * lp.grid) || d_ckpt_dump.alloc(lp.dump_total))
                return -1;
            LaunchArgs a;
            a.kp = kparams.p; a.seqs = seqs.dev; a.jobs = d_jobs.p; a.n_jobs = n; a.results = d_results.p;
            a.seqs.sub_colptr = nullptr; a.seqs.sub_rows = nullptr;
            a.seqs.span_in = nullptr; a.seqs.span_out = nullptr;
            if (span) {                                      // matrices of all jobs, in job order
                std::vector<int> host(lp.span_total);
                for (int x = 0; x < n; x++) {
                    const JobSpec &sp = specs[order[x]];
                    const int32_t *src = span == 1 ? sp.span_in : sp.span_out;
                    const long long cnt = (long long)(jobs[x].Q + 1) * (jobs[x].T + 1) * span_cs;
                    memcpy(host.data() + jobs[x].span_off, src, sizeof(int) * cnt);
                }
                if (d_span.upload(host.data(), lp.span_total, s)) return -1;
                a.seqs.span_in = d_span.p; a.seqs.span_out = d_span.p;
            }
            if (pts) {
                lp.sub_q.push_back(0);                      // the kernels' row prefetch may touch one entry past the last list
                if (d_sub_t.upload(lp.sub_t.data(), lp.sub_t.size(), s) || d_sub_q.upload(lp.sub_q.data(), lp.sub_q.size(), s) ||
                    d_sub_colptr.alloc(2 * lp.sub_cols)) return -1;
                hipLaunchKernelGGL(subopt_colptr_kernel, dim3(std::min(n, 65535)), dim3(256), 0, s, d_jobs.p, n,
                                   d_sub_t.p, d_sub_q.p, d_sub_colptr.p);
                HIP_OK(hipGetLastError());
                a.seqs.sub_colptr = d_sub_colptr.p; a.seqs.sub_rows = d_sub_q.p;
            }
            a.seqs.ss16 = seqs.ss16_built ? seqs.ss16.p : nullptr;
            if (seed && seed->mode == 2 && seed->fmt16) {
                // the packed windows' dense target codes and code table ride in the two pointers no packed kernel reads otherwise
                if (seqs.tdense_n <= 0) { c4h::set_error("packed region windows without a residue-code table"); return -1; }
                a.seqs.sub_rows = reinterpret_cast<const int *>(seqs.tcode_dense.p);
                a.seqs.sub_colptr = reinterpret_cast<const int *>(seqs.tdense.p);
            }
            a.seqs.seed = nullptr;
            if (seed) {
                if (seed->mode == 1 && d_seed.alloc((size_t)std::max<long long>(lp.seed_total, 1))) return -1;
                a.seqs.seed = d_seed.p;
            }
            a.vsas = d_vsa.p; a.ops = nullptr; a.queue = d_queue.p; a.grid = (int)lp.grid; a.stream = s;
            if (ki->pairs) {
                if (d_pairs.upload(lp.pair_list.data(), lp.pair_list.size(), s)) return -1;
                a.aux = d_pairs.p; a.n_aux = (int)(lp.pair_list.size() / 2);
            }
            if (staged_codes) a.aux = reinterpret_cast<const int *>(staged_codes);
            a.scratch.bnd = d_bnd.p; a.scratch.bnd_stride = lp.bnd_per_wave; a.scratch.carry = lp.carry_T ? 1 : 0;
            a.scratch.tb = lp.max_tb ? d_tb.p : nullptr; a.scratch.tb_stride = lp.max_tb;
            a.scratch.ckpt = lp.max_ckpt ? d_ckpt.p : nullptr; a.scratch.ckpt_stride = lp.max_ckpt;
            a.scratch.ckpt_dump = d_ckpt_dump.p;
            a.scratch.runs = d_runs.p; a.scratch.runs_stride = lp.max_runs;
            a.scratch.runs_out = d_runs_out.p; a.scratch.runs_capacity = runs_capacity;
            a.scratch.runs_used = d_runs_used.p;
            tr.lap("uploaded");
            if (ctx->timing) HIP_OK(hipEventRecord(ctx->ev0, s));
            HIP_OK(ki->launch(a));
            if (ctx->timing) HIP_OK(hipEventRecord(ctx->ev1, s));
            unsigned long long used = 0;
            if (d_results.download(res.data(), n, s) || d_runs_used.download(&used, 1, s) ||
                d_vsa.download(vsa.data(), lp.vsa_total, s) || d_ckpt_dump.download(dump.data(), lp.dump_total, s))
                return -1;
            HIP_OK(c4_stream_sync(s));
            tr.lap("kernel + results");
            if (ctx->timing) {
                float ms = 0;
                HIP_OK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
                ctx->kernel_ms[mode] += ms; ctx->kernel_launches[mode]++; ctx->kernel_cells[mode] += lp.total_cells;
            }
            if ((long long)used > runs_capacity) {          // rare: paths with very short runs
                if (attempt == 1) { c4h::set_error("traceback runs exceed their worst-case buffer"); return -1; }
                runs_capacity = lp.ops_total;
                continue;
            }
            runs.resize(used);
            if (d_runs_out.download(runs.data(), used, s)) return -1;
            HIP_OK(c4_stream_sync(s));
            if (span == 2) {                                 // END cells back into the callers' matrices
                std::vector<int> host(lp.span_total);
                if (d_span.download(host.data(), lp.span_total, s)) return -1;
                HIP_OK(c4_stream_sync(s));
                for (int x = 0; x < n; x++) {
                    const long long cnt = (long long)(jobs[x].Q + 1) * (jobs[x].T + 1) * span_cs;
                    memcpy(specs[order[x]].span_out, host.data() + jobs[x].span_off, sizeof(int) * cnt);
                }
            }
            break;
        }
        return 0;
    }

    // the results of launch_jobs, per job, into the caller's order
    int unpack(int mode, const KernelInfo *ki, int n, std::vector<JobOut> &out) {
        const std::vector<int> &order = h_order, &dump = h_dump;
        const std::vector<DevJob> &jobs = h_jobs;
        const std::vector<DevResult> &res = h_res;
        const std::vector<uint32_t> &runs = h_runs;
        const std::vector<DevVsa> &vsa = h_vsa;
        std::atomic<int> overflow{0};
        parallel_for(n, 32768, [&](long long first, long long last) {
            for (long long x = first; x < last; x++) {
                JobOut &o = out[order[x]];
                o.res = res[x];
                if (res[x].flags & FLAG_OPS_OVERFLOW) { overflow = 1; continue; }
                if (mode == MODE_PATH) o.runs.assign_reversed(runs.data() + res[x].ops_off, res[x].n_ops);   // the walk wrote END -> START
                else o.runs.n = 0;
                if (mode == MODE_CKPT) o.vsa.assign(vsa.begin() + jobs[x].vsa_off, vsa.begin() + jobs[x].vsa_off + res[x].n_vsa);
                else o.vsa.clear();
                if (mode == MODE_CKPT && jobs[x].ckpt_off >= 0) {
                    const long long ck = (long long)jobs[x].cp_count * ki->max_at * (jobs[x].Q + 1) * ki->n_states * ki->cs;
                    o.checkpoints.assign(dump.begin() + jobs[x].ckpt_off, dump.begin() + jobs[x].ckpt_off + ck);
                } else {
                    o.checkpoints.clear();
                }
            }
        });
        if (overflow) { c4h::set_error("traceback path longer than its buffer"); return -1; }
        return 0;
    }
};
