// c4_engine_find_path.inc -- part of c4_engine.hip (one translation unit; included there, in this order): Optimal_find_path over a batch (optimal.c:368-413): region, checkpoints, sub-alignments, verification and repair of predicted cells; the two launch lanes.
// subs (may be NULL): per-pair SubOpt, the `subopt` argument the reference hands to every Viterbi_calculate of
// the path (optimal.c:368-413); active (may be NULL): pairs to run, the others get no alignment.
// initial (may be NULL): the `region` argument of each pair's Optimal_find_path (default: the whole rectangle) — what
// GAM_Result_refine_alignment passes for --refine region (gam.c:618-640).
int find_path_batch(Engine &eng, const ResidentSeqs &seqs, int dpmemory_mb, c4gpu_score threshold,
                    c4gpu_alignment *alignments, const std::vector<const c4gpu_subopt *> *subs = nullptr,
                    const uint8_t *active = nullptr, const std::vector<c4gpu_score> *pair_thresholds = nullptr,
                    const c4gpu_region *initial = nullptr, bool own_all = true) {
    // own_all = false: one of two lanes working on the same arrays (find_path_lanes): only the entries of `active` are this
    // call's to touch, and the caller has cleared them
    const c4gpu_model *m = eng.model;
    const int n = seqs.n_pairs;
    // per-pair thresholds (GAM_get_query_threshold with --percent, gam.c:677-705): never below `threshold`
    const c4gpu_score base_threshold = threshold;
    auto thr = [&](int pair) {
        return (pair_thresholds && (*pair_thresholds)[pair] > base_threshold) ? (*pair_thresholds)[pair] : base_threshold;
    };
    struct SubScope {                // every eng.run below sees the pairs' blocked cells
        Engine &e;
        SubScope(Engine &e_, const std::vector<const c4gpu_subopt *> *s) : e(e_) { e.pair_sub = s; }
        ~SubScope() { e.pair_sub = nullptr; }
    } sub_scope(eng, subs);
    const bool trace = c4cfg::has(c4cfg::TRACE);
    const auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (trace) fprintf(stderr, "c4gpu trace: find_path_batch: %-28s at %.3f ms\n", what,
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    };
    const bool strict_cells = cell_strict();
    std::vector<PairPlan> plan(n);
    std::vector<JobSpec> &specs = eng.fp_specs;
    std::vector<JobOut> &outs = eng.fp_outs;
    specs.clear();
    std::vector<int> owner;
    if (own_all) for (int i = 0; i < n; i++) memset(&alignments[i], 0, sizeof(c4gpu_alignment));
    // -- step 1: where the whole rectangle is too large for a traceback, find the region first
    std::vector<int> region_pairs;
    for (int i = 0; i < n; i++) {
        plan[i].ar = initial ? initial[i] : c4gpu_region{0, 0, seqs.qlen[i], seqs.tlen[i]};
        plan[i].active = !active || active[i];
        if (!plan[i].active) continue;
        if (c4h::use_reduced_space(m, &plan[i].ar, dpmemory_mb)) {
            plan[i].reduced = true;
            if (!model_is_global(m)) region_pairs.push_back(i);        // Optimal_find_region, optimal.c:135
        }
    }
    const size_t step1_total = region_pairs.size();
    double &hit_rate = eng.ctx->hit_rate[subs ? 1 : 0];
    // long targets under a local model, nothing blocked: the two-pass (windowed) form of the region pass
    std::vector<std::pair<int, DevResult>> region_done;
    {
        // a dump every 8 192 columns (measured on the north-star batch with 32-bit dumps: score pass 410 ms against 462 ms at 4 096,
        // windows 204 against 181 ms; 16 384: 408 and 272 ms), every 4 096 while some target of the call is too short for that
        // -- and where the packed score pass serves, whose 16-bit dump rows cost it 1.4 ms per launch more at 4 096 while the
        // windows save 9 (step on two lanes 442 -> 436 ms; 2 048: 438; profiles/r04_kshift_sweep.log)
        // (4 096 only where the packed pass will really run: a call with a pair that does not fit its 16 bits -- a long query, a
        // small --intronpenalty -- or with C4GPU_PK16=0 dumps 32-bit rows, for which 8 192 is the better interval)
        bool pk16_serves = pk16_enabled(eng.family, eng.pk16_params_ok, (long long)region_pairs.size(), Switches::from_config());
        for (size_t x = 0; x < region_pairs.size() && pk16_serves; x++)
            pk16_serves = eng.pk16_fits(plan[region_pairs[x]].ar.query_length, plan[region_pairs[x]].ar.target_length);
        int kshift_env = pk16_serves ? 12 : 13;
        for (int i : region_pairs)
            if (plan[i].ar.target_length < (4 << 13) && plan[i].ar.target_length >= (4 << 12)) kshift_env = 12;
        kshift_env = c4cfg::num(c4cfg::SEED_KSHIFT, kshift_env);
        const int kshift = std::max(2, std::min(kshift_env, 20));
        const bool off = c4cfg::is(c4cfg::WINDOWED, 0);
        const KernelInfo *k1 = get_kernel_mw(eng.family, MODE_SCORE, true, false, 4, false, 1);
        const KernelInfo *k2 = get_kernel_mw(eng.family, MODE_REGION, true, true, 4, false, 2);
        // where most alignments ran past the hop budget in the earlier batches of this context (chance alignments across
        // whole windows: all-against-all without a threshold), the one-pass kernel is the cheaper form
        const bool pays = eng.ctx->window_rate < 0 || eng.ctx->window_rate >= 0.5 || c4cfg::has(c4cfg::SEED_KSHIFT);
        if (!off && pays && !subs && eng.local && eng.local_exact && k1 && k2 && !(c4cfg::is(c4cfg::PACK, 0))) {
            std::vector<int> win_pairs, rest;
            for (int i : region_pairs) {
                const c4gpu_region &ar = plan[i].ar;
                const bool rows_ok = ar.query_length + 1 > 2 * 64 * k2->R;       // the cooperating-wave kernels' domain
                if (rows_ok && ar.target_length >= (4 << kshift) && ar.query_length < (1 << 20)) win_pairs.push_back(i);
                else rest.push_back(i);
            }
            if (!win_pairs.empty()) {
                std::vector<DevResult> wres;
                if (windowed_region_pass(eng, seqs, win_pairs, plan, thr, kshift, wres)) return -1;
                for (size_t x = 0; x < win_pairs.size(); x++) region_done.emplace_back(win_pairs[x], wres[x]);
                region_pairs.swap(rest);
            }
        }
    }
    // A pair whose best score is below the threshold ends here (optimal.c:144-145).  The score alone costs
    // 0.64 of a region pass (no region-start payload), so where few pairs reach the threshold — all-vs-all
    // runs, the last round of the sub-optimal loop — a FIND_SCORE pass goes first and only the survivors get
    // the region pass.  Same recurrence, same score (FIND_SCORE and FIND_REGION differ in payload only); the
    // choice follows the hit rate of the previous batches of this context, sampled on the first large one.
    {
        const bool sf_env = c4cfg::has(c4cfg::SCORE_FIRST);                // 0 never, 1 always, unset adaptive
        const bool can = threshold > C4GPU_IMPOSSIBLY_LOW_SCORE && region_pairs.size() >= 512;
        const size_t total = region_pairs.size();
        auto score_filter = [&](size_t first, size_t count, size_t *kept) -> int {
            specs.clear();
            for (size_t x = first; x < first + count; x++) { JobSpec s; s.pair = region_pairs[x]; s.region = plan[region_pairs[x]].ar; specs.push_back(s); }
            if (eng.run(seqs, MODE_SCORE, false, specs, outs)) return -1;
            *kept = 0;
            for (size_t x = 0; x < count; x++) {
                if (outs[x].res.score < thr(region_pairs[first + x])) plan[region_pairs[first + x]].active = false;
                else (*kept)++;
            }
            return 0;
        };
        bool score_first = false;
        size_t sampled = 0, kept = 0, all_kept = 0;
        if (can && sf_env) score_first = c4cfg::num(c4cfg::SCORE_FIRST, 0) != 0;
        else if (can && hit_rate >= 0) score_first = hit_rate < 0.3;
        else if (can) {
            // one device-filling launch costs about the same as a small one: sample that many pairs
            sampled = std::min<size_t>(8 * (size_t)eng.ctx->prop.multiProcessorCount, total);
            if (score_filter(0, sampled, &kept)) return -1;
            all_kept = kept;
            score_first = (double)kept / (double)sampled < 0.3;
        }
        if (score_first && sampled < total) {
            if (score_filter(sampled, total - sampled, &kept)) return -1;
            all_kept += kept;
        }
        if (score_first || sampled) {
            std::vector<int> survivors;
            for (int i : region_pairs) if (plan[i].active) survivors.push_back(i);
            region_pairs.swap(survivors);
        }
        (void)all_kept;
    }
    specs.clear();
    for (int i : region_pairs) { JobSpec s; s.pair = i; s.region = plan[i].ar; specs.push_back(s); }
    if (eng.run(seqs, MODE_REGION, false, specs, outs)) return -1;
    for (size_t x = 0; x < region_pairs.size(); x++) region_done.emplace_back(region_pairs[x], outs[x].res);
    for (const auto &pr : region_done) {
        PairPlan &p = plan[pr.first];
        const DevResult &r = pr.second;
        if (r.score < thr(pr.first)) { p.active = false; continue; }
        p.region_score = r.score;
        p.end_from = r.last_srp;                 // the windowed pass's packed score kernel reports it (c4_viterbi16_kernel.h); else 0
        // Viterbi_Data_finalise, viterbi.c:633-653 (curr_*_start are relative to the region the pass ran over)
        if (m->start_scope != C4GPU_SCOPE_QUERY) p.ar.query_start += r.qs;
        if (m->start_scope != C4GPU_SCOPE_TARGET) p.ar.target_start += r.ts;
        p.ar.query_length = r.qe - (m->start_scope != C4GPU_SCOPE_QUERY ? r.qs : 0);
        p.ar.target_length = r.te - (m->start_scope != C4GPU_SCOPE_TARGET ? r.ts : 0);
    }
    if (step1_total >= 64 && threshold > C4GPU_IMPOSSIBLY_LOW_SCORE) {
        size_t hits = 0;
        for (const auto &pr : region_done) hits += plan[pr.first].active ? 1 : 0;
        const double rate = (double)hits / (double)step1_total;
        hit_rate = hit_rate < 0 ? rate : 0.5 * hit_rate + 0.5 * rate;
    }
    lap("region pass done");
    // -- step 2: quadratic-space path wherever the (alignment) region fits (optimal.c:349-364, 382-390)
    specs.clear(); owner.clear();
    for (int i = 0; i < n; i++) {
        PairPlan &p = plan[i];
        if (!p.active) continue;
        if (p.reduced && c4h::use_reduced_space(m, &p.ar, dpmemory_mb)) continue;
        p.reduced = false;
        JobSpec s; s.pair = i; s.region = p.ar;
        specs.push_back(s); owner.push_back(i);
    }
    if (eng.run(seqs, MODE_PATH, false, specs, outs)) return -1;
    for (size_t x = 0; x < owner.size(); x++) {
        const int i = owner[x];
        const DevResult &r = outs[x].res;
        c4gpu_alignment &a = alignments[i];
        a.score = r.score;
        // Viterbi_Data_create_Alignment, viterbi.c:380-383
        a.region.query_start = plan[i].ar.query_start + r.qs;
        a.region.target_start = plan[i].ar.target_start + r.ts;
        a.region.query_length = r.qe - r.qs;
        a.region.target_length = r.te - r.ts;
        int cap = 0;
        for (uint32_t r : outs[x].runs) c4h::alignment_add(&a, &cap, (int)(r >> 24), (int)(r & 0xffffff));
        a.valid = 1;
    }
    lap("quadratic paths done");
    // -- step 3: reduced space: checkpoint passes, recursively (optimal.c:160-230,315-345)
    std::vector<int> red;
    for (int i = 0; i < n; i++)
        if (plan[i].active && plan[i].reduced) {
            Segment s;
            memset(&s, 0, sizeof s);
            s.region = plan[i].ar; s.first_state = m->start_state; s.needs_checkpoints = true;
            plan[i].segs.assign(1, s);
            red.push_back(i);
        }
    std::map<int, JobOut> ckpt_done;            // first checkpoint pass of the pairs the device route left over
    if (!red.empty() && !subs) {
        // the device route first: whatever it finishes leaves the list
        std::vector<char> done(n, 0);
        if (fused_reduced_paths(eng, seqs, red, plan, dpmemory_mb, alignments, done, ckpt_done)) return -1;
        std::vector<int> rest;
        for (int i : red) if (!done[i]) rest.push_back(i);
        red.swap(rest);
        lap("device route done");
    }
    std::vector<c4gpu_score> red_score(n, 0);
    std::vector<char> redo(n, 0), packed_pair(n, 0);        // packed_pair: predicted cells from the packed checkpoint pass
    for (const auto &kv : ckpt_done) packed_pair[kv.first] = kv.second.packed ? 1 : 0;
    bool first_round = true;
    for (;;) {
        struct Ref { int pair, seg; };
        std::vector<Ref> refs;
        specs.clear();
        for (int i : red) {
            std::vector<Segment> &sg = plan[i].segs;
            for (size_t k = 0; k < sg.size(); k++) {
                if (!sg[k].needs_checkpoints) continue;
                JobSpec s; s.pair = i; s.region = sg[k].region;
                s.first_state = sg[k].first_state;
                // optimal.c:204-213: first cell = final cell of the previous sub-alignment (or the zero cell),
                // final state = first state of the next one (or END)
                if (k > 0) memcpy(s.first_cell, sg[k - 1].final_cell, sizeof s.first_cell);
                s.final_state = (k + 1 < sg.size()) ? sg[k + 1].first_state : m->end_state;
                s.cp_count = c4h::checkpoint_rows(m, &s.region, dpmemory_mb);
                specs.push_back(s);
                refs.push_back(Ref{i, (int)k});
            }
        }
        if (specs.empty()) break;
        lap("checkpoint jobs listed");
        bool have_all = first_round && !ckpt_done.empty();
        for (size_t x = 0; x < refs.size() && have_all; x++) have_all = ckpt_done.count(refs[x].pair) != 0;
        if (have_all) {                              // the device route ran exactly these jobs: its results are this round's
            if (outs.size() < refs.size()) outs.resize(refs.size());
            for (size_t x = 0; x < refs.size(); x++) outs[x] = ckpt_done[refs[x].pair];
        } else if (eng.run(seqs, MODE_CKPT, true, specs, outs)) return -1;
        lap("checkpoint pass done");
        // expand from the back so that segment indices stay valid; the jobs of one pair are adjacent in the list and
        // pairs do not touch each other's segments
        std::vector<int> group;
        for (size_t x = 0; x < refs.size(); x++)
            if (!x || refs[x].pair != refs[x - 1].pair) group.push_back((int)x);
        group.push_back((int)refs.size());
        parallel_for((long long)group.size() - 1, 256, [&](long long g0, long long g1) {
          for (long long g = g0; g < g1; g++)
            for (int x = group[g + 1] - 1; x >= group[g]; x--) {
            std::vector<Segment> &sg = plan[refs[x].pair].segs;
            const int k = refs[x].seg;
            if (first_round) red_score[refs[x].pair] = outs[x].res.score;
            std::vector<Segment> children;
            children.reserve(outs[x].vsa.size());
            for (int v = (int)outs[x].vsa.size() - 1; v >= 0; v--) {     // path order = reverse of the list
                const DevVsa &dv = outs[x].vsa[v];
                Segment c;
                c.region = c4gpu_region{dv.qs, dv.ts, dv.ql, dv.tl};
                c.first_state = dv.first_state;
                memcpy(c.final_cell, dv.final_cell, sizeof c.final_cell);
                c.needs_checkpoints = c4h::use_reduced_space(m, &c.region, dpmemory_mb);
                children.push_back(c);
            }
            // optimal.c:214-217 passes vsa->final_cell as the buffer the recursive pass overwrites; siblings
            // scheduled in the same round used the old value: it must not have changed
            if (!first_round && !children.empty() &&
                !final_cell_equiv(children.back().final_cell, sg[k].final_cell, 1 + m->total_shadow_designations,
                                  sg[k].region.target_start + sg[k].region.target_length, packed_pair[refs[x].pair] != 0, strict_cells)) {
                // Who has used the old value?  Only a sibling whose own nested pass ran in this round seeded with it: the
                // segment right behind this one, if it is a checkpoint job of this round too.  Every other use lies ahead --
                // the sub-alignment pass of step 4 seeds segment k + 1 with the cell the nested pass has just written (what
                // optimal.c:283,301 does) and verifies every final cell against its prediction there -- so only that case
                // sends the pair down the call-by-call route (one launch per section: 50 launches of 2 ms for a chance
                // alignment across a 100 kb window, profiles/r05_wide_trace.md).
                const bool next_in_round = x + 1 < group[g + 1] && refs[x + 1].seg == k + 1;
                if (c4cfg::has(c4cfg::TRACE))
                    fprintf(stderr, "c4gpu trace: pair %d nested segment %d: final cell %d/%d after the nested pass, %d/%d predicted%s\n",
                            refs[x].pair, k, children.back().final_cell[0], children.back().final_cell[1], sg[k].final_cell[0], sg[k].final_cell[1],
                            next_in_round ? ": the next segment's nested pass used the old cell, sequential route" : "");
                if (next_in_round || c4cfg::nonzero(c4cfg::NESTED_REDO)) redo[refs[x].pair] = 1;
            }
            sg.erase(sg.begin() + k);
            sg.insert(sg.begin() + k, children.begin(), children.end());
            }
        });
        first_round = false;
    }
    lap("segments expanded");
    // -- step 4: the sub-alignments themselves (Optimal_compute_subalignments, optimal.c:266-313)
    specs.clear();
    struct Ref2 { int pair, seg; };
    std::vector<Ref2> refs2;
    std::vector<size_t> seg_first(red.size() + 1, 0);          // first sub-alignment job of each reduced-space pair
    for (size_t r = 0; r < red.size(); r++) seg_first[r + 1] = seg_first[r] + plan[red[r]].segs.size();
    std::vector<JobSpec> &sub_specs = eng.fp_sub_specs;
    if (sub_specs.size() != seg_first[red.size()]) sub_specs.resize(seg_first[red.size()]);
    refs2.resize(seg_first[red.size()]);
    parallel_for((long long)red.size(), 256, [&](long long r0, long long r1) {
        for (long long r = r0; r < r1; r++) {
            const int i = red[r];
            const std::vector<Segment> &sg = plan[i].segs;
            for (size_t k = 0; k < sg.size(); k++) {
                JobSpec s; s.pair = i; s.region = sg[k].region;
                s.first_state = sg[k].first_state;
                if (k > 0) memcpy(s.first_cell, sg[k - 1].final_cell, sizeof s.first_cell);
                s.final_state = (k + 1 < sg.size()) ? sg[k + 1].first_state : m->end_state;
                sub_specs[seg_first[r] + k] = s;
                refs2[seg_first[r] + k] = Ref2{i, (int)k};
            }
        }
    });
    lap("sub-alignment jobs listed");
    if (eng.run(seqs, MODE_PATH, true, sub_specs, outs)) return -1;
    lap("sub-alignment pass done");
    {
        std::vector<int> cap(n, 0);
        const int path_cs = 1 + m->total_shadow_designations;
        const bool force_seq = c4cfg::has(c4cfg::FORCE_SEQUENTIAL);    // test hook
        if (force_seq) for (int i : red) redo[i] = 1;
        // The reference threads the final cell of each sub-DP into the next one (optimal.c:283,301); we
        // predicted it from the checkpoint rows to run all sub-DPs in one launch.  Verify: up to and including
        // the first sub-alignment whose final cell differs from the prediction, the batch did what the
        // reference does; the ones after it were seeded with a cell the reference would not have used.
        struct Repair { int pair, next_seg; int seed[CELL_MAX]; };
        std::vector<Repair> repairs;
        std::vector<int> repairing(n, -1);                 // first sub-alignment to recompute, per pair
        std::mutex repairs_lock;
        parallel_for((long long)red.size(), 256, [&](long long r0, long long r1) {
          for (long long r = r0; r < r1; r++)
            for (size_t x = seg_first[r]; x < seg_first[r + 1]; x++) {
            const int i = refs2[x].pair, k = refs2[x].seg;
            c4gpu_alignment &a = alignments[i];
            std::vector<Segment> &sg = plan[i].segs;
            if (k == 0) {
                a.score = red_score[i];
                a.region = plan[i].ar;
                a.valid = 1;
            }
            if (redo[i] || repairing[i] >= 0) continue;     // redone below from the first stale sub-alignment
            for (uint32_t r : outs[x].runs) c4h::alignment_add(&a, &cap[i], (int)(r >> 24), (int)(r & 0xffffff));
            if (!final_cell_equiv(outs[x].res.final_cell, sg[k].final_cell, path_cs,
                                  sg[k].region.target_start + sg[k].region.target_length, packed_pair[i] != 0, strict_cells)) {
                if (c4cfg::has(c4cfg::TRACE))
                    fprintf(stderr, "c4gpu trace: pair %d sub-alignment %d: final cell %d/%d computed, %d/%d predicted\n", i,
                            k, outs[x].res.final_cell[0], outs[x].res.final_cell[1], sg[k].final_cell[0], sg[k].final_cell[1]);
                if (k + 1 < (int)sg.size()) {
                    Repair rp; rp.pair = i; rp.next_seg = k + 1;
                    memcpy(rp.seed, outs[x].res.final_cell, sizeof rp.seed);
                    std::lock_guard<std::mutex> hold(repairs_lock);
                    repairs.push_back(rp);
                    repairing[i] = k + 1;
                }
            }
            }
        });
        // the repair launches below take the pairs in list order
        std::sort(repairs.begin(), repairs.end(), [](const Repair &x, const Repair &y) { return x.pair < y.pair; });
        // Optimal_compute_subalignments (optimal.c:266-313) for the stale tails, all affected pairs in lock-step: one small
        // launch per sub-alignment that has to be recomputed, seeded with the cell its predecessor actually produced.  A
        // recomputed sub-alignment that ends in the cell the batch had PREDICTED for it re-joins the batch: the sub-alignments
        // behind it were seeded with exactly that cell, so what the batch computed for them is what the reference computes
        // (same inputs), up to the next one whose final cell differs -- where the next repair starts.  (Without this a miss
        // early in a wide region cost one launch per remaining section: 50 launches of 2 ms for a chance alignment across a
        // 100 kb window, profiles/r05_wide_trace.md; differences in a cell are mostly an intron start that the next match
        // state forgets.)  C4GPU_REPAIR_REJOIN=0: recompute every sub-alignment behind a miss (test hook).
        const bool rejoin = !(c4cfg::is(c4cfg::REPAIR_REJOIN, 0));
        std::vector<size_t> first_of(n, 0);
        for (size_t r = 0; r < red.size(); r++) first_of[red[r]] = seg_first[r];
        std::vector<JobOut> routs;
        long long repair_launches = 0, repaired = 0, rejoined = 0;
        while (!repairs.empty()) {
            specs.clear();
            for (const Repair &rp : repairs) {
                const std::vector<Segment> &sg = plan[rp.pair].segs;
                JobSpec s; s.pair = rp.pair; s.region = sg[rp.next_seg].region;
                s.first_state = sg[rp.next_seg].first_state;
                memcpy(s.first_cell, rp.seed, sizeof s.first_cell);
                s.final_state = (rp.next_seg + 1 < (int)sg.size()) ? sg[rp.next_seg + 1].first_state : m->end_state;
                specs.push_back(s);
            }
            if (eng.run(seqs, MODE_PATH, true, specs, routs)) return -1;
            repair_launches++; repaired += (long long)repairs.size();
            std::vector<Repair> next;
            for (size_t x = 0; x < repairs.size(); x++) {
                Repair rp = repairs[x];
                c4gpu_alignment &a = alignments[rp.pair];
                const std::vector<Segment> &sg = plan[rp.pair].segs;
                const int nseg = (int)sg.size();
                for (uint32_t r : routs[x].runs) c4h::alignment_add(&a, &cap[rp.pair], (int)(r >> 24), (int)(r & 0xffffff));
                memcpy(rp.seed, routs[x].res.final_cell, sizeof rp.seed);
                const int j = rp.next_seg;
                if (j + 1 >= nseg) continue;
                const bool joined = rejoin && final_cell_equiv(rp.seed, sg[j].final_cell, path_cs,
                                                               sg[j].region.target_start + sg[j].region.target_length, packed_pair[rp.pair] != 0, strict_cells);
                if (!joined) { rp.next_seg = j + 1; next.push_back(rp); continue; }
                rejoined++;
                // the batch's own results from j + 1 on, up to (and including) the next sub-alignment that misses its prediction
                for (int k = j + 1; k < nseg; k++) {
                    const JobOut &bo = outs[first_of[rp.pair] + k];
                    for (uint32_t r : bo.runs) c4h::alignment_add(&a, &cap[rp.pair], (int)(r >> 24), (int)(r & 0xffffff));
                    if (k + 1 < nseg && !final_cell_equiv(bo.res.final_cell, sg[k].final_cell, path_cs,
                                                          sg[k].region.target_start + sg[k].region.target_length, packed_pair[rp.pair] != 0, strict_cells)) {
                        rp.next_seg = k + 1;
                        memcpy(rp.seed, bo.res.final_cell, sizeof rp.seed);
                        next.push_back(rp);
                        break;
                    }
                }
            }
            repairs.swap(next);
        }
        if (repair_launches && c4cfg::has(c4cfg::TRACE))
            fprintf(stderr, "c4gpu trace: stale tails: %lld sub-alignments recomputed in %lld launches, %lld re-joined the batch\n",
                    repaired, repair_launches, rejoined);
    }
    lap("alignments assembled");
    for (int i : red)
        if (redo[i] && sequential_reduced_path(eng, seqs, i, dpmemory_mb, plan[i].ar, &alignments[i])) return -1;
    for (int i = 0; i < n; i++) {
        if (active && !active[i]) continue;
        c4gpu_alignment &a = alignments[i];
        if (a.valid && a.score < thr(i)) c4gpu_alignment_clear(&a);     // optimal.c:408-411
    }
    return 0;
}

// ---- two launch lanes ---------------------------------------------------------------------------------------------
// The passes of Optimal_find_path are persistent kernels that end in a tail: the last round of jobs leaves part of the
// device idle (the packed score pass of the north-star batch runs 2 048 lane pairs on 768 resident workgroups: 2.67
// rounds), the windows and the checkpoint pass likewise.  A large batch is therefore cut into two halves of equal work
// that walk through the passes on two streams from two host threads: the workgroups of one half's next pass start as the
// other half's tail drains (measured on the north-star batch: 928 -> 839 ms per step; four lanes: 1 036 ms).  Both lanes
// read the same resident sequences; each has its own stream, events, statistics and launch buffers.  C4GPU_LANES=1
// keeps one lane, =2 forces two.
struct SideLane {
    c4gpu_ctx ctx;
    Engine eng;
    ~SideLane() {
        if (ctx.stream) (void)hipStreamDestroy(ctx.stream);
        if (ctx.ev0) (void)hipEventDestroy(ctx.ev0);
        if (ctx.ev1) (void)hipEventDestroy(ctx.ev1);
    }
    int init(const c4gpu_ctx *main, const c4gpu_model *m, const c4gpu_params *p) {
        ctx.device = main->device; ctx.prop = main->prop; ctx.timing = main->timing;
        HIP_OK(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
        HIP_OK(hipEventCreate(&ctx.ev0));
        HIP_OK(hipEventCreate(&ctx.ev1));
        if (eng.init(&ctx, m, p)) return -1;
        HIP_OK(c4_stream_sync(ctx.stream));
        return 0;
    }
};

// would this call be cut in two?  (callers create the side lane only then)
bool lanes_wanted(const ResidentSeqs &seqs, const uint8_t *active, bool blocking) {
    const int env = c4cfg::num(c4cfg::LANES, 0);
    if (blocking || env == 1) return false;
    long long n_act = 0;
    double cells = 0;
    for (int i = 0; i < seqs.n_pairs; i++) {
        if (active && !active[i]) continue;
        n_act++;
        cells += (double)(seqs.qlen[i] + 1) * (double)(seqs.tlen[i] + 1);
    }
    if (env == 2) return n_act >= 2;
    // each half must still fill the device more than once with whole-rectangle jobs that take long enough to have a tail
    return n_act >= 2048 && cells / (double)n_act >= 2.0e6;
}

int find_path_lanes(Engine &eng, SideLane *side, const ResidentSeqs &seqs, int dpmemory_mb, c4gpu_score threshold,
                    c4gpu_alignment *alignments, const uint8_t *active = nullptr,
                    const std::vector<c4gpu_score> *pair_thresholds = nullptr, const c4gpu_region *initial = nullptr) {
    const int n = seqs.n_pairs;
    if (!side || eng.annotated || !lanes_wanted(seqs, active, false))
        return find_path_batch(eng, seqs, dpmemory_mb, threshold, alignments, nullptr, active, pair_thresholds, initial);
    // equal work per lane: every pair goes to the lane with fewer first-pass cells so far
    std::vector<uint8_t> mask[2] = {std::vector<uint8_t>(n, 0), std::vector<uint8_t>(n, 0)};
    double load[2] = {0, 0};
    for (int i = 0; i < n; i++) {
        if (active && !active[i]) continue;
        const int l = load[1] < load[0] ? 1 : 0;
        mask[l][i] = 1;
        load[l] += (double)((initial ? initial[i].query_length : seqs.qlen[i]) + 1) * (double)((initial ? initial[i].target_length : seqs.tlen[i]) + 1);
    }
    for (int i = 0; i < n; i++) memset(&alignments[i], 0, sizeof(c4gpu_alignment));
    side->ctx.timing = eng.ctx->timing;
    int r1 = 0;
    std::string err1;
    const int device = eng.ctx->device;
    // an exception (std::bad_alloc of a host vector) must neither leave the second thread nor skip its join
    std::thread second([&] {
        try {
            if (hipSetDevice(device) != hipSuccess) { r1 = -1; err1 = "hipSetDevice on the second lane"; return; }
            r1 = find_path_batch(side->eng, seqs, dpmemory_mb, threshold, alignments, nullptr, mask[1].data(), pair_thresholds, initial, false);
            if (r1) err1 = c4h::g_error;
        } catch (const std::exception &e) { r1 = -1; err1 = std::string("second launch lane: ") + e.what(); }
    });
    int r0 = 0;
    try {
        r0 = find_path_batch(eng, seqs, dpmemory_mb, threshold, alignments, nullptr, mask[0].data(), pair_thresholds, initial, false);
    } catch (const std::exception &e) { r0 = -1; c4h::set_error(std::string("first launch lane: ") + e.what()); }
    second.join();
    if (r0) return r0;
    if (r1) { c4h::set_error(err1); return r1; }
    return 0;
}

