// c4_seed_dev.inc — the word scan of the seeder on the device (part of c4_engine.hip: it uses c4gpu_ctx and DevBuf).
//
// The reference's Seeder_add_target (src/comparison/seeder.c:852-915) walks every target (for translated matches: the
// three translated frames) through the automaton its queries built (FSM_traverse, src/struct/fsm.c:186-198; the compact
// form: Seeder_VFSM_traverse_single, seeder.c:698-720) and calls Seeder_FSM_traverse_func (seeder.c:649-695) wherever a
// word ends: one dependent pointer load per target residue on one host core.  All words of a seeder have one length W
// (FSM_add is only ever called with hsp_param->wordlen, seeder.c:199-203), so the compiled automaton — failure links and
// all — reports exactly the positions whose last W symbols spell a word of the table, and a symbol outside the alphabet
// (column 0) resets it.  Here: the word table as a hash from the W-symbol code to (first emission, emissions) in device
// memory; one thread per target position computes the code of the W-mer that ends there and looks it up; an exclusive
// prefix sum over the per-position emission counts gives every hit its place, so the hit list comes out in the
// reference's order — position ascending, then the word's emission order (its own seeds, then its neighbours' seeds) —
// without a sort.  Bytes: the symbol string once (n), the counts (4 n written, read once), 8 bytes per hit.

namespace {

struct WordSlot { unsigned long long code; int first, count; };

__host__ __device__ __forceinline__ unsigned long long word_hash(unsigned long long c) {
    c ^= c >> 31; c *= 0x9E3779B97F4A7C15ull; c ^= c >> 29;
    return c;
}

// The kernels below that scan or reduce run 256 threads with 8 items each; part: 256 entries of LDS.
constexpr int SEED_ITEMS = 8;

// the sum over the block (in thread 0 only)
template <class T> __device__ __forceinline__ T block_sum(T mine, T *part) {
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    return part[0];
}

// the sum over the threads in front of this one (Hillis-Steele)
template <class T> __device__ __forceinline__ T block_exclusive_scan(T mine, T *part) {
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const T add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    return part[threadIdx.x] - mine;
}

// cnt[i] = emissions of the word whose last symbol is symbols[i] (0: no word ends there); blocksum[b] = their sum per block
__global__ __launch_bounds__(256) void seed_count_kernel(const uint8_t *__restrict__ sym, int n, int width, int wordlen,
                                                         const WordSlot *__restrict__ slots, unsigned mask,
                                                         int *__restrict__ cnt, int *__restrict__ first,
                                                         unsigned long long *__restrict__ blocksum) {
    __shared__ unsigned long long part[256];
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * SEED_ITEMS;
    unsigned long long mine = 0;
    for (int k = 0; k < SEED_ITEMS; k++) {
        const long long i = base + k;
        if (i >= n) break;
        int c = 0, f = 0;
        if (i >= wordlen - 1) {
            unsigned long long code = 0;
            bool ok = true;
            for (int w = 0; w < wordlen; w++) {
                const unsigned s = sym[i - wordlen + 1 + w];
                ok &= s != 0;
                code = code * (unsigned)width + s;
            }
            if (ok) {
                unsigned h = (unsigned)word_hash(code) & mask;
                for (;;) {
                    const WordSlot e = slots[h];
                    if (e.count == 0) break;
                    if (e.code == code) { c = e.count; f = e.first; break; }
                    h = (h + 1) & mask;
                }
            }
        }
        cnt[i] = c; first[i] = f;
        mine += (unsigned)c;
    }
    const unsigned long long sum = block_sum(mine, part);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = sum;
}

// exclusive prefix sum of the block sums, one workgroup
__global__ __launch_bounds__(1024) void seed_blockscan_kernel(unsigned long long *blocksum, int n_blocks, unsigned long long *total) {
    __shared__ unsigned long long part[1024];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_blocks; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long v = i < n_blocks ? blocksum[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {                     // inclusive scan (Hillis-Steele)
            const unsigned long long add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n_blocks) blocksum[i] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// A thread's positions and their hits, every hit with its place: hit_base + block offset + the prefix inside the block.
// emit(position, emission, place)
template <class Emit>
__device__ __forceinline__ void seed_walk_hits(int n, const int *__restrict__ cnt, const int *__restrict__ first,
                                               unsigned long long hit_base, Emit emit) {
    __shared__ unsigned long long part[256];
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * SEED_ITEMS;
    unsigned long long mine = 0;
    for (int k = 0; k < SEED_ITEMS; k++) if (base + k < n) mine += (unsigned)cnt[base + k];
    unsigned long long pos = hit_base + block_exclusive_scan(mine, part);
    for (int k = 0; k < SEED_ITEMS; k++) {
        const long long i = base + k;
        if (i >= n) break;
        const int c = cnt[i], f = first[i];
        for (int e = 0; e < c; e++, pos++) emit((int)i, f + e, pos);
    }
}

// the hit list of c4gpu_seed_scan
__global__ __launch_bounds__(256) void seed_fill_kernel(int n, const int *__restrict__ cnt, const int *__restrict__ first,
                                                        const unsigned long long *__restrict__ blockoff,
                                                        c4gpu_word_hit *__restrict__ hits, unsigned long long cap) {
    seed_walk_hits(n, cnt, first, blockoff[blockIdx.x], [&](int i, int emission, unsigned long long pos) {
        if (pos < cap) hits[pos] = c4gpu_word_hit{i, emission};
    });
}

// ---- c4gpu_seed_extend: the hits stay here and become the HSPs a fresh HSPset per pair would store ---------------------
// The scan above gives every hit its walk index; what HSPset_seed_hsp (hspset.c:933-997) then does hit by hit depends on the
// order only through the horizon entry the seed is tested against (:939-958) and moves (:990).  So: every hit becomes a seed
// with the number of its entry (its slot: all entries of all pairs numbered through, slot_base[pair] + (section * aq + qf) * at
// + tf, or n_slots for a seed without one); a stable radix sort groups the walk indices by slot, walk order kept inside a slot; one
// lane per run of equal slots replays that entry alone (hsp_entry_step, c4_hsp_extend.h); a prefix sum over the kept
// verdicts in walk-index order lays the kept HSPs out as HSP_store met them.  c4gpu_seed_extend_opt: the same for soft-masked
// sets (the two-stage extension, a dropped seed's masked end as its entry's horizon, :981-995) and --seedrepeat > 1 (the entry
// also carries its counter and diagonal tag, :950-970); what an entry holds still depends on that entry's seeds alone.

// the same walk with the seed and its slot in place of the hit
__global__ __launch_bounds__(256) void seed_expand_kernel(int n, const int *__restrict__ cnt, const int *__restrict__ first,
                                                          const unsigned long long *__restrict__ blockoff, unsigned long long hit_base,
                                                          unsigned long long n_hits, const c4gpu_seed_emit *__restrict__ emits,
                                                          const HspJob *__restrict__ jobs, const unsigned *__restrict__ slot_base,
                                                          int scale, int offset, int modifier, int aq, int at, int seedlen,
                                                          unsigned n_slots,
                                                          c4gpu_hsp_seed *__restrict__ seeds, unsigned *__restrict__ keys,
                                                          int *__restrict__ vals, unsigned long long *__restrict__ outside,
                                                          unsigned long long *__restrict__ first_hit) {
    seed_walk_hits(n, cnt, first, hit_base + blockoff[blockIdx.x], [&](int i, int emission, unsigned long long pos) {
        if (pos >= n_hits) return;
        const int ts = i * scale + offset - modifier;
        const c4gpu_seed_emit em = emits[emission];
        const HspJob jb = jobs[em.pair];
        if (pos < first_hit[em.pair]) atomicMin(&first_hit[em.pair], pos);      // (it only ever falls: a stale read is too large)
        unsigned key = n_slots;
        int pair = em.pair;
        if (ts < 0 || jb.qlen <= 0 || (long long)em.query_pos + (long long)seedlen * aq > jb.qlen ||
            (long long)ts + (long long)seedlen * at > jb.tlen) {
            *outside = 1;                                            // the call fails; the seed is never read through
            pair = -1;
        } else if (aq == 1) {
            const int diag = ts - em.query_pos * at;                 // hspset.c:941-944 (query advance 1)
            const int section = (diag + jb.qlen) % jb.qlen;          // C's remainder: negative above the main diagonal's reach
            if (section >= 0) key = slot_base[em.pair] + (unsigned)section * (unsigned)at + (unsigned)(ts % at);
        } else {
            // both advances 3 (CODON2CODON).  Sequence.len is unsigned, so the reference's sum and remainder are (hspset.c:935-943):
            // a seed more than qlen under the main diagonal wraps to an entry another diagonal owns, and has one like any other
            const unsigned sum = (unsigned)ts * (unsigned)aq - (unsigned)em.query_pos * (unsigned)at + (unsigned)jb.qlen;
            const unsigned section = sum % (unsigned)jb.qlen;
            key = slot_base[em.pair] + (section * (unsigned)aq + (unsigned)(em.query_pos % aq)) * (unsigned)at + (unsigned)(ts % at);
        }
        seeds[pos] = c4gpu_hsp_seed{pair, em.query_pos, ts};
        keys[pos] = key;
        vals[pos] = (int)pos;
    });
}

// LSD radix sort, 8 bits a pass, one wave per tile of 2048: digit histogram (hist[digit * n_blocks + block], so that one
// exclusive scan over the whole array -- seed_blockscan_kernel -- is every (digit, block)'s place), then a stable scatter
constexpr int SEED_SORT_TILE = 64 * 32;

// (K: unsigned for the horizon slots; unsigned long long for the word codes of c4_wordtab_build.inc)
template <class K>
__global__ __launch_bounds__(64) void seed_sort_hist_kernel(const K *__restrict__ keys, long long n, int shift, int n_blocks,
                                                            unsigned long long *__restrict__ hist) {
    __shared__ unsigned h[256];
    for (int x = threadIdx.x; x < 256; x += 64) h[x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * SEED_SORT_TILE;
    for (int k = 0; k < 32; k++) {
        const long long i = base + k * 64 + threadIdx.x;
        if (i < n) atomicAdd(&h[(unsigned)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < 256; x += 64) hist[(size_t)x * n_blocks + blockIdx.x] = h[x];
}

template <class K>
__global__ __launch_bounds__(64) void seed_sort_scatter_kernel(const K *__restrict__ keys, const int *__restrict__ vals, long long n,
                                                               int shift, int n_blocks, const unsigned long long *__restrict__ hist,
                                                               K *__restrict__ keys_out, int *__restrict__ vals_out) {
    __shared__ unsigned long long off[256];
    for (int x = threadIdx.x; x < 256; x += 64) off[x] = hist[(size_t)x * n_blocks + blockIdx.x];
    __syncthreads();
    const unsigned long long below = (1ull << threadIdx.x) - 1;         // the lanes in front of this one
    const long long base = (long long)blockIdx.x * SEED_SORT_TILE;
    for (int k = 0; k < 32; k++) {                                       // 64 keys at a time, in order: stable
        const long long i = base + k * 64 + threadIdx.x;
        const bool active = i < n;
        const K key = active ? keys[i] : (K)0;
        const unsigned d = (unsigned)(key >> shift) & 255u;
        unsigned long long same = __ballot(active);                      // the active lanes that hold this lane's digit
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long set = __ballot(active && bit);
            same &= bit ? set : ~set;
        }
        unsigned long long dst = 0;
        if (active) dst = off[d] + (unsigned)__popcll(same & below);
        __syncthreads();
        if (active && !(same & below)) off[d] += (unsigned)__popcll(same);
        __syncthreads();
        if (active && dst < (unsigned long long)n) { keys_out[dst] = key; vals_out[dst] = vals[i]; }
    }
}

// One lane per run of equal slots in the sorted list (a seed without a horizon entry is a run of its own): HSPset_seed_hsp
// seed by seed on that entry alone (hsp_entry_step, c4_hsp_extend.h).  verdict[k] of walk index k: 0 not extended (under the
// horizon, or under REPEAT held back by the entry's counter), 1 extended and not kept (below the threshold; under MASKED also
// a seed dropped after its forbidding round, hsps[k] then its masked end), 2 kept.  MASKED: a.qmask / a.tmask are read.
// REPEAT: seed_repeat > 1, the entry carries its counter and diagonal tag; every seed has an entry then (refused otherwise).
template <bool MASKED, bool REPEAT>
__global__ void seed_chain_kernel(const HspArgs a, const c4gpu_hsp_seed *__restrict__ seeds, const unsigned *__restrict__ keys,
                                  const int *__restrict__ order, long long n, unsigned n_slots, int seed_repeat,
                                  const int *__restrict__ submat, uint8_t *__restrict__ verdict, c4gpu_hsp *__restrict__ hsps) {
    __shared__ int sm[24 * 24];
    hsp_load_matrix(sm, submat);
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < n; x += (long long)gridDim.x * blockDim.x) {
        const unsigned key = keys[x];
        const bool entry = key != n_slots;
        if (entry && x > 0 && keys[x - 1] == key) continue;              // not the first of its run
        HspEntry e{0, 0, 0};                                             // a fresh set's entries start at 0: no seed (their
        for (long long y = x; y < n && keys[y] == key; y++) {            // target_start >= 0) lies below, with an entry or not
            const int k = order[y];
            const c4gpu_hsp_seed sd = seeds[k];
            c4gpu_hsp h;
            int dropped = 0;
            if (sd.pair < 0 || !hsp_entry_step_as<MASKED, REPEAT>(a, sm, sd, seed_repeat, e, &h, MASKED ? &dropped : nullptr))
                verdict[k] = 0;
            else {
                hsps[k] = h;
                verdict[k] = !dropped && h.score >= a.threshold ? 2 : 1; // HSP_store
            }
            if (!entry) break;
        }
    }
}

// kept HSPs per block of 2048 walk indices (for the prefix sum) and the number of extended seeds below the threshold
__global__ __launch_bounds__(256) void seed_verdict_count_kernel(const uint8_t *__restrict__ verdict, long long n,
                                                                 unsigned long long *__restrict__ blocksum,
                                                                 unsigned long long *__restrict__ n_below) {
    __shared__ unsigned kept[256], under[256];
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * SEED_ITEMS;
    unsigned a = 0, b = 0;
    for (int k = 0; k < SEED_ITEMS; k++)
        if (base + k < n) { const int v = verdict[base + k]; a += v == 2; b += v == 1; }
    a = block_sum(a, kept); b = block_sum(b, under);
    if (threadIdx.x == 0) {
        blocksum[blockIdx.x] = a;
        if (b) atomicAdd(n_below, (unsigned long long)b);
    }
}

// the kept HSPs to their places, in walk-index order
__global__ __launch_bounds__(256) void seed_compact_kernel(const uint8_t *__restrict__ verdict, long long n,
                                                           const unsigned long long *__restrict__ blockoff,
                                                           const c4gpu_hsp_seed *__restrict__ seeds, const c4gpu_hsp *__restrict__ hsps,
                                                           c4gpu_seed_hsp *__restrict__ out, unsigned long long cap) {
    __shared__ unsigned part[256];
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * SEED_ITEMS;
    unsigned mine = 0;
    for (int k = 0; k < SEED_ITEMS; k++) if (base + k < n) mine += verdict[base + k] == 2;
    unsigned long long pos = blockoff[blockIdx.x] + block_exclusive_scan(mine, part);
    for (int k = 0; k < SEED_ITEMS; k++) {
        const long long i = base + k;
        if (i >= n) break;
        if (verdict[i] != 2) continue;
        if (pos < cap) out[pos] = c4gpu_seed_hsp{(int64_t)i, seeds[i].pair, hsps[i]};
        pos++;
    }
}

}  // namespace

struct c4gpu_wordtab {
    c4gpu_ctx *ctx;
    int width, wordlen, n_words;
    int n_emissions = 0;                   // emit_first[n_words]: what c4gpu_wordtab_set_emissions must bring
    unsigned mask;
    DevBuf<WordSlot> slots;
    // c4gpu_seed_extend: the emissions (c4gpu_wordtab_set_emissions) and its scratch
    bool emits_set = false;
    int emit_max_pair = -1;
    DevBuf<c4gpu_seed_emit> d_emits;
    DevBuf<c4gpu_hsp_seed> d_seeds;
    DevBuf<unsigned> d_keys[2], d_slot_base;
    DevBuf<int> d_vals[2], d_submat;
    DevBuf<unsigned long long> d_hist, d_report, d_first_hit;
    int first_hit_pairs = -1;              // pairs of the last c4gpu_seed_extend call (-1: none yet), and whether it had hits
    bool first_hit_any = false;
    DevBuf<uint8_t> d_verdict;
    DevBuf<c4gpu_hsp> d_hsps;
    DevBuf<c4gpu_seed_hsp> d_out;
    DevBuf<HspJob> d_jobs;
    DevBuf<uint8_t> d_qmask, d_tmask;      // c4gpu_seed_extend_opt: the soft masks of the flagged sides (softmask_kernel)
    // scratch kept between scans of one seeder (targets of similar size follow each other)
    DevBuf<uint8_t> d_sym;
    DevBuf<int> d_cnt, d_first;
    DevBuf<unsigned long long> d_blocksum, d_total;
    DevBuf<c4gpu_word_hit> d_hits;
    double scan_ms = 0;
    long long scans = 0, symbols = 0, hits = 0;
    // c4gpu_wordtab_export: the words by code ascending with their first emissions (n_words + 1 entries).  A table built on the
    // device (c4gpu_wordtab_build) keeps them there, one made by c4gpu_wordtab_create keeps what the caller gave
    bool built = false;
    DevBuf<unsigned long long> d_codes;
    DevBuf<int> d_emit_first;
    std::vector<uint64_t> h_codes;
    std::vector<int32_t> h_first;
};

extern "C" c4gpu_wordtab *c4gpu_wordtab_create(c4gpu_ctx *ctx, int32_t width, int32_t wordlen, const uint64_t *codes,
                                               const int32_t *emit_first, int32_t n_words) {
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return nullptr; }
    if (width < 2 || width > 255 || wordlen < 1 || wordlen > 32 || n_words < 0) { c4h::set_error("word table: bad shape"); return nullptr; }
    double span = 1;
    for (int w = 0; w < wordlen; w++) span *= width;
    if (span > 1.8e19) { c4h::set_error("word table: width^wordlen does not fit 64 bits"); return nullptr; }
    try {
        std::unique_ptr<c4gpu_wordtab> t(new c4gpu_wordtab);
        t->ctx = ctx; t->width = width; t->wordlen = wordlen; t->n_words = n_words;
        t->n_emissions = n_words > 0 ? emit_first[n_words] : 0;
        t->h_codes.assign(codes, codes + n_words);
        if (n_words > 0) t->h_first.assign(emit_first, emit_first + n_words + 1);
        unsigned size = 16;
        while (size < 2u * (unsigned)std::max(1, n_words)) size <<= 1;
        t->mask = size - 1;
        std::vector<WordSlot> host(size, WordSlot{0, 0, 0});
        for (int k = 0; k < n_words; k++) {
            const int count = emit_first[k + 1] - emit_first[k];
            if (count <= 0) continue;                                   // a word without emissions reports nothing
            unsigned h = (unsigned)word_hash(codes[k]) & t->mask;
            while (host[h].count) {
                if (host[h].code == codes[k]) { c4h::set_error("word table: a word listed twice"); return nullptr; }
                h = (h + 1) & t->mask;
            }
            host[h] = WordSlot{codes[k], emit_first[k], count};
        }
        if (t->slots.upload(host.data(), size, ctx->stream)) return nullptr;
        if (c4_stream_sync(ctx->stream) != hipSuccess) { c4h::set_error("word table upload failed"); return nullptr; }
        return t.release();
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_wordtab_create: ") + e.what());
        return nullptr;
    }
}

extern "C" void c4gpu_wordtab_destroy(c4gpu_wordtab *t) { delete t; }

// The count stage over the n symbols at d_sym + sym_off: emissions and first emission per position (d_cnt, d_first, same
// offset), the exclusive prefix of the per-block sums at d_blocksum + blk_off and their total in d_total[total_at].
static int seed_count_blocks(long long n) { return (int)((n + 256 * SEED_ITEMS - 1) / (256 * SEED_ITEMS)); }
static void seed_count_launch(c4gpu_wordtab *t, hipStream_t s, size_t sym_off, int n, size_t blk_off, size_t total_at) {
    const int n_blocks = seed_count_blocks(n);
    hipLaunchKernelGGL(seed_count_kernel, dim3(n_blocks), dim3(256), 0, s, t->d_sym.p + sym_off, n, t->width, t->wordlen, t->slots.p,
                       t->mask, t->d_cnt.p + sym_off, t->d_first.p + sym_off, t->d_blocksum.p + blk_off);
    hipLaunchKernelGGL(seed_blockscan_kernel, dim3(1), dim3(1024), 0, s, t->d_blocksum.p + blk_off, n_blocks, t->d_total.p + total_at);
}

extern "C" int c4gpu_seed_scan(c4gpu_ctx *ctx, c4gpu_wordtab *t, const uint8_t *symbols, int32_t n, c4gpu_word_hit *hits,
                               int64_t cap, int64_t *n_hits) {
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return -1; }
    *n_hits = 0;
    if (n <= 0) return 0;
    hipStream_t s = ctx->stream;
    const int n_blocks = seed_count_blocks(n);
    // C4GPU_TRACE: where a scan's wall time goes, call by call (a scan beside another thread's long kernel: r05)
    const bool laps_on = c4cfg::has(c4cfg::TRACE);
    auto lap_t = std::chrono::steady_clock::now();
    char laps[256]; int laps_n = 0; laps[0] = 0;
    auto lap = [&](const char *what) {
        if (!laps_on) return;
        const auto u = std::chrono::steady_clock::now();
        laps_n += snprintf(laps + laps_n, sizeof laps - laps_n, " %s %.2f", what, std::chrono::duration<double, std::milli>(u - lap_t).count());
        if (laps_n > (int)sizeof laps - 1) laps_n = (int)sizeof laps - 1;
        lap_t = u;
    };
    if (t->d_sym.upload(symbols, (size_t)n, s)) return -1;
    lap("upload");
    if ( t->d_cnt.alloc(n) || t->d_first.alloc(n) || t->d_blocksum.alloc(n_blocks) ||
        t->d_total.alloc(1) || t->d_hits.alloc((size_t)std::max<int64_t>(cap, 1))) return -1;
    lap("allocs");
    HIP_OK(hipEventRecord(ctx->ev0, s));
    seed_count_launch(t, s, 0, n, 0, 0);
    hipLaunchKernelGGL(seed_fill_kernel, dim3(n_blocks), dim3(256), 0, s, n, t->d_cnt.p, t->d_first.p, t->d_blocksum.p, t->d_hits.p,
                       (unsigned long long)std::max<int64_t>(cap, 0));
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(ctx->ev1, s));
    unsigned long long total = 0;
    lap("launches");
    if (t->d_total.download(&total, 1, s)) return -1;
    HIP_OK(c4_stream_sync(s));
    lap("sync");
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    t->scan_ms += ms; t->scans++; t->symbols += n; t->hits += (long long)total;
    *n_hits = (int64_t)total;
    if ((int64_t)total > cap) return 0;                                 // the caller comes back with room for all of them
    if (total) { if (t->d_hits.download(hits, (size_t)total, s)) return -1; HIP_OK(c4_stream_sync(s)); }
    lap("hits");
    if (laps_on) fprintf(stderr, "c4gpu trace: seed scan of %d symbols (ms):%s; kernels %.2f\n", n, laps, ms);
    return 0;
}

extern "C" void c4gpu_wordtab_stats(const c4gpu_wordtab *t, double *scan_ms, int64_t *scans, int64_t *symbols, int64_t *hits) {
    if (scan_ms) *scan_ms = t->scan_ms;
    if (scans) *scans = t->scans;
    if (symbols) *symbols = t->symbols;
    if (hits) *hits = t->hits;
}

extern "C" int c4gpu_wordtab_set_emissions(c4gpu_wordtab *t, const c4gpu_seed_emit *emits, int32_t n_emits) {
    c4gpu_ctx *ctx = t->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return -1; }
    t->emits_set = false;
    if (n_emits != t->n_emissions) {
        c4h::set_error("c4gpu_wordtab_set_emissions: the table's words report " + std::to_string(t->n_emissions) + " emissions, " +
                       std::to_string(n_emits) + " given");
        return -1;
    }
    int max_pair = -1;
    for (int e = 0; e < n_emits; e++) {
        if (emits[e].pair < 0 || emits[e].query_pos < 0) {
            c4h::set_error("c4gpu_wordtab_set_emissions: an emission names a negative pair or query position");
            return -1;
        }
        max_pair = std::max(max_pair, emits[e].pair);
    }
    if (t->d_emits.upload(emits, (size_t)n_emits, ctx->stream)) return -1;
    HIP_OK(c4_stream_sync(ctx->stream));
    t->emits_set = true;
    t->emit_max_pair = max_pair;
    return 0;
}

extern "C" int c4gpu_seed_extend_opt(c4gpu_ctx *ctx, c4gpu_wordtab *t, const c4gpu_params *params, int match_type,
                                     const c4gpu_pair *pairs, int32_t n_pairs, const uint8_t *const *symbols, const int32_t *n_symbols,
                                     int32_t n_strings, int32_t tpos_scale, const int32_t *tpos_offset, int32_t tpos_modifier,
                                     int32_t seedlen, int32_t dropoff, int32_t threshold, int32_t mask_query, int32_t mask_target,
                                     int32_t seed_repeat, c4gpu_seed_hsp *out, int64_t cap, c4gpu_seed_extend_stats *stats) {
    try {
        *stats = c4gpu_seed_extend_stats{0, 0, 0, 0};
        if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return -1; }
        if (!hsp_match_known(match_type)) { c4h::set_error("unknown match type"); return -1; }
        if (seed_repeat < 1) { c4h::set_error("c4gpu_seed_extend: seed_repeat below 1"); return -1; }
        if (seed_repeat > 1 && match_type == C4GPU_MATCH_PROTEIN2DNA) {
            c4h::set_error("c4gpu_seed_extend: seed_repeat above 1 is not served for PROTEIN2DNA (seeds without a horizon entry)");
            return -1;
        }
        if (!t->emits_set) { c4h::set_error("c4gpu_seed_extend: no emissions set (c4gpu_wordtab_set_emissions)"); return -1; }
        if (t->emit_max_pair >= n_pairs) { c4h::set_error("c4gpu_seed_extend: an emission names a pair outside `pairs`"); return -1; }
        if (n_pairs < 0 || n_strings < 0 || tpos_scale < 1 || seedlen < 1) { c4h::set_error("c4gpu_seed_extend: bad shape"); return -1; }
        for (int i = 1; i < n_pairs; i++)
            if (pairs[i].target != pairs[0].target || pairs[i].target_len != pairs[0].target_len) {
                c4h::set_error("c4gpu_seed_extend: the pairs do not all name one target buffer and length");
                return -1;
            }
        const int aq = hsp_query_advance(match_type), at = hsp_target_advance(match_type);
        long long n_slots = 0;
        std::vector<unsigned> slot_base((size_t)std::max(1, n_pairs));
        for (int i = 0; i < n_pairs; i++) {
            slot_base[i] = (unsigned)n_slots;
            n_slots += (long long)std::max(0, pairs[i].query_len) * aq * at;
            if (n_slots > 0x7fffffffLL) { c4h::set_error("c4gpu_seed_extend: more than 2^31 - 1 horizon entries"); return -1; }
        }
        // the strings behind each other in one buffer, each with whole count blocks of its own
        std::vector<size_t> sym_off((size_t)n_strings + 1, 0), blk_off((size_t)n_strings + 1, 0);
        for (int s = 0; s < n_strings; s++) {
            const int n = std::max(0, n_symbols[s]);
            sym_off[s + 1] = sym_off[s] + (size_t)n;
            blk_off[s + 1] = blk_off[s] + (size_t)seed_count_blocks(n);
        }
        const size_t total_sym = sym_off[n_strings];
        t->first_hit_pairs = n_pairs; t->first_hit_any = false;
        if (!total_sym || !n_pairs || !t->n_emissions) return 0;
        ResidentSeqs seqs;
        if (seqs.build(ctx, hsp_family(match_type), params, pairs, n_pairs)) return -1;
        const std::vector<HspJob> jobs = hsp_jobs(seqs, n_pairs);
        hipStream_t s = ctx->stream;
        std::vector<unsigned long long> totals((size_t)n_strings, 0), hit_base((size_t)n_strings + 1, 0);
        std::vector<uint8_t> hsym(total_sym);
        for (int k = 0; k < n_strings; k++)
            if (sym_off[k + 1] > sym_off[k]) memcpy(hsym.data() + sym_off[k], symbols[k], sym_off[k + 1] - sym_off[k]);
        if (t->d_jobs.upload(jobs.data(), n_pairs, s) || t->d_slot_base.upload(slot_base.data(), n_pairs, s) ||
            t->d_submat.upload(hsp_matrix(params, match_type), 24 * 24, s) || t->d_sym.upload(hsym.data(), total_sym, s) || t->d_cnt.alloc(total_sym) ||
            t->d_first.alloc(total_sym) || t->d_blocksum.alloc(blk_off[n_strings]) || t->d_total.upload(totals.data(), (size_t)n_strings, s)) return -1;
        // 1. count, per string
        for (int k = 0; k < n_strings; k++)
            if (sym_off[k + 1] > sym_off[k]) seed_count_launch(t, s, sym_off[k], (int)(sym_off[k + 1] - sym_off[k]), blk_off[k], k);
        HIP_OK(hipGetLastError());
        if (t->d_total.download(totals.data(), (size_t)n_strings, s)) return -1;     // 8 bytes per string: they size the buffers
        HIP_OK(c4_stream_sync(s));
        for (int k = 0; k < n_strings; k++) hit_base[k + 1] = hit_base[k] + totals[k];
        const unsigned long long n_hits = hit_base[n_strings];
        t->scans += n_strings; t->symbols += (long long)total_sym; t->hits += (long long)n_hits;
        stats->n_hits = (int64_t)n_hits;
        if (n_hits > 0x7fffffffULL) { c4h::set_error("c4gpu_seed_extend: more than 2^31 - 1 word hits"); return -1; }
        if (!n_hits) return 0;
        const long long N = (long long)n_hits;
        const int n_tiles = (int)((N + SEED_SORT_TILE - 1) / SEED_SORT_TILE);          // sort tiles and verdict blocks: 2048 each
        const unsigned long long cap_dev = (unsigned long long)std::min<long long>(std::max<int64_t>(cap, 0), N);
        const unsigned long long zero4[4] = {0, 0, 0, 0};                             // outside flag, below, kept, (scan scratch)
        if (t->d_seeds.alloc(N) || t->d_keys[0].alloc(N) || t->d_keys[1].alloc(N) || t->d_vals[0].alloc(N) || t->d_vals[1].alloc(N) ||
            t->d_verdict.alloc(N) || t->d_hsps.alloc(N) || t->d_hist.alloc((size_t)256 * n_tiles) || t->d_report.upload(zero4, 4, s) ||
            t->d_out.alloc((size_t)std::max<unsigned long long>(cap_dev, 1))) return -1;
        {
            const std::vector<unsigned long long> none((size_t)n_pairs, ~0ull);
            if (t->d_first_hit.upload(none.data(), (size_t)n_pairs, s)) return -1;
            HIP_OK(c4_stream_sync(s));                                                // (`none` goes away)
        }
        // 2. expand
        for (int k = 0; k < n_strings; k++) {
            const int n = (int)(sym_off[k + 1] - sym_off[k]), n_blocks = (int)(blk_off[k + 1] - blk_off[k]);
            if (!n || !totals[k]) continue;
            hipLaunchKernelGGL(seed_expand_kernel, dim3(n_blocks), dim3(256), 0, s, n, t->d_cnt.p + sym_off[k], t->d_first.p + sym_off[k],
                               t->d_blocksum.p + blk_off[k], hit_base[k], n_hits, t->d_emits.p, t->d_jobs.p, t->d_slot_base.p, tpos_scale,
                               tpos_offset ? tpos_offset[k] : 0, tpos_modifier, aq, at, seedlen, (unsigned)n_slots, t->d_seeds.p,
                               t->d_keys[0].p, t->d_vals[0].p, t->d_report.p, t->d_first_hit.p);
        }
        // 3. group by slot: keys run to n_slots (the seeds without an entry)
        int passes = 0, cur = 0;
        for (unsigned long long v = (unsigned long long)n_slots; v; v >>= 8) passes++;
        for (int p = 0; p < passes; p++, cur ^= 1) {
            hipLaunchKernelGGL(seed_sort_hist_kernel<unsigned>, dim3(n_tiles), dim3(64), 0, s, t->d_keys[cur].p, N, 8 * p, n_tiles, t->d_hist.p);
            hipLaunchKernelGGL(seed_blockscan_kernel, dim3(1), dim3(1024), 0, s, t->d_hist.p, 256 * n_tiles, t->d_report.p + 3);
            hipLaunchKernelGGL(seed_sort_scatter_kernel<unsigned>, dim3(n_tiles), dim3(64), 0, s, t->d_keys[cur].p, t->d_vals[cur].p, N, 8 * p, n_tiles,
                               t->d_hist.p, t->d_keys[cur ^ 1].p, t->d_vals[cur ^ 1].p);
        }
        // the masks of the flagged sides, from the raw residues the batch keeps (the 64 bytes of padding included: hsp_extend_host)
        const bool masked = mask_query || mask_target, repeat = seed_repeat > 1;
        const uint8_t *qmask = nullptr, *tmask = nullptr;
        if (mask_query) {
            const long long hq_n = seqs.total_q + 64;
            if (t->d_qmask.alloc((size_t)hq_n)) return -1;
            hipLaunchKernelGGL(softmask_kernel, dim3(1024), dim3(256), 0, s, seqs.qraw.p, t->d_qmask.p, hq_n, aq,
                               match_type == C4GPU_MATCH_DNA2DNA || match_type == C4GPU_MATCH_CODON2CODON ? 'n' : 'x');
            qmask = t->d_qmask.p;
        }
        if (mask_target) {
            const long long ht_n = seqs.total_t + 64;
            if (t->d_tmask.alloc((size_t)ht_n)) return -1;
            hipLaunchKernelGGL(softmask_kernel, dim3(1024), dim3(256), 0, s, seqs.traw.p, t->d_tmask.p, ht_n, at,
                               match_type == C4GPU_MATCH_PROTEIN2PROTEIN ? 'x' : 'n');
            tmask = t->d_tmask.p;
        }
        // 4. chains, 5. compaction
        const int chain_grid = (int)std::min<long long>((N + 63) / 64, 1 << 20);
        const HspArgs a{seqs.qcode.p, seqs.tcode.p, qmask, tmask, t->d_jobs.p, aq, at, seedlen, dropoff, threshold};
        const auto chain_kernel = masked ? (repeat ? seed_chain_kernel<true, true> : seed_chain_kernel<true, false>)
                                         : (repeat ? seed_chain_kernel<false, true> : seed_chain_kernel<false, false>);
        hipLaunchKernelGGL(chain_kernel, dim3(chain_grid), dim3(64), 0, s, a, t->d_seeds.p, t->d_keys[cur].p, t->d_vals[cur].p, N,
                           (unsigned)n_slots, seed_repeat, t->d_submat.p, t->d_verdict.p, t->d_hsps.p);
        hipLaunchKernelGGL(seed_verdict_count_kernel, dim3(n_tiles), dim3(256), 0, s, t->d_verdict.p, N, t->d_hist.p, t->d_report.p + 1);
        hipLaunchKernelGGL(seed_blockscan_kernel, dim3(1), dim3(1024), 0, s, t->d_hist.p, n_tiles, t->d_report.p + 2);
        hipLaunchKernelGGL(seed_compact_kernel, dim3(n_tiles), dim3(256), 0, s, t->d_verdict.p, N, t->d_hist.p, t->d_seeds.p, t->d_hsps.p,
                           t->d_out.p, cap_dev);
        HIP_OK(hipGetLastError());
        unsigned long long report[3] = {0, 0, 0};
        if (t->d_report.download(report, 3, s)) return -1;
        HIP_OK(c4_stream_sync(s));
        if (report[0]) { c4h::set_error("c4gpu_seed_extend: a seed does not lie inside its pair"); return -1; }
        t->first_hit_any = true;
        stats->n_below = (int64_t)report[1];
        stats->n_kept = (int64_t)report[2];
        stats->n_extended = stats->n_below + stats->n_kept;
        if (stats->n_kept > cap) return 0;                                  // the caller comes back with room for all of them
        if (stats->n_kept) { if (t->d_out.download(out, (size_t)stats->n_kept, s)) return -1; HIP_OK(c4_stream_sync(s)); }
        return 0;
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_seed_extend: ") + e.what());
        return -1;
    }
}

extern "C" int c4gpu_seed_extend(c4gpu_ctx *ctx, c4gpu_wordtab *t, const c4gpu_params *params, int match_type,
                                 const c4gpu_pair *pairs, int32_t n_pairs, const uint8_t *const *symbols, const int32_t *n_symbols,
                                 int32_t n_strings, int32_t tpos_scale, const int32_t *tpos_offset, int32_t tpos_modifier,
                                 int32_t seedlen, int32_t dropoff, int32_t threshold, c4gpu_seed_hsp *out, int64_t cap,
                                 c4gpu_seed_extend_stats *stats) {
    return c4gpu_seed_extend_opt(ctx, t, params, match_type, pairs, n_pairs, symbols, n_symbols, n_strings, tpos_scale, tpos_offset,
                                 tpos_modifier, seedlen, dropoff, threshold, 0, 0, 1, out, cap, stats);
}

extern "C" int c4gpu_seed_extend_first_hits(c4gpu_ctx *ctx, c4gpu_wordtab *t, int64_t *first_hit, int32_t n_pairs) {
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return -1; }
    if (t->first_hit_pairs < 0 || n_pairs != t->first_hit_pairs) {
        c4h::set_error("c4gpu_seed_extend_first_hits: no c4gpu_seed_extend call over that many pairs came before");
        return -1;
    }
    for (int i = 0; i < n_pairs; i++) first_hit[i] = -1;
    if (!t->first_hit_any || !n_pairs) return 0;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "first hits are downloaded in place");
    if (t->d_first_hit.download(reinterpret_cast<unsigned long long *>(first_hit), (size_t)n_pairs, ctx->stream)) return -1;
    HIP_OK(c4_stream_sync(ctx->stream));                                              // (no hit: ~0 is -1)
    return 0;
}

#include "c4_wordtab_build.inc"
