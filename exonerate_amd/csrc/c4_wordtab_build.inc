// c4_wordtab_build.inc — the seeder's word table built on the device from the queries themselves (included by c4_seed_dev.inc).
//
// The reference builds it on one host core: Seeder_add_query -> Seeder_load_query -> Seeder_insert_query
// (src/comparison/seeder.c:478-558) puts every word of every query into the automaton, prepends its seed to the word's seed list
// (seeder.c:103-107) and, when a word gets its FIRST seed (seeder.c:546-553), walks its neighbourhood (WordHood_traverse,
// src/comparison/wordhood.c:192-218,277-299,321-341) and prepends the word to the neighbour list of every word in it
// (Seeder_WordHood_traverse, seeder.c:461-476; :121-124).  What a scan then reports for a word N is its own seeds followed by the
// whole seed list of every neighbour (Seeder_FSM_traverse_func, seeder.c:674-692).  In closed form, with the occurrences numbered
// g = 0, 1, ... in insertion order:
//   own(c)   = the seeds of the occurrences of code c, g descending
//   first(W) = the smallest g of W;  hood(W) = the words the pruned walk reaches from W, W itself left out
//   emissions(N) = own(N), then own(W) for every W with N in hood(W), first(W) descending
// Here, all on the device, sizes (five counts) the only thing the host reads on the way:
//   1. occurrences: one thread per symbol; a prefix sum over the "a word ends here" flags numbers them       -> (code, g), seed[g]
//   2. the stable radix sort of c4_seed_dev.inc on the 64-bit code: a run of equal codes is a seeded word, its head first(W), the
//      run read backwards own(W); a prefix sum over "g is a first occurrence" ranks the seeded words by first(W)
//   3. neighbourhoods, one wave per seeded word, the waves in rank-DESCENDING order: count per lane, prefix sum, the same walk
//      again writes (code N, wave).  The link list is therefore already sorted by first(W) descending,
//   4. and one stable sort on the code leaves it sorted by (code ascending, first(W) descending)
//   5. seeded codes and link targets merge into the word list (binary searches + a prefix sum over the new codes), a prefix sum
//      over the list lengths is emit_first, one wave per word copies its lists, and the WordSlots go into the hash by
//      compare-and-swap on the code (a slot's content depends on its code alone).
// Every order above comes from a prefix sum or a stable sort: two builds give the same bytes.

namespace {

// ---- prefix sums over int arrays: per-block sums, seed_blockscan_kernel over them, then the places -------------------------
__global__ __launch_bounds__(256) void wt_blocksum_kernel(const int *__restrict__ cnt, long long n, unsigned long long *__restrict__ blocksum) {
    __shared__ unsigned long long part[256];
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * SEED_ITEMS;
    unsigned long long mine = 0;
    for (int k = 0; k < SEED_ITEMS; k++) if (base + k < n) mine += (unsigned)cnt[base + k];
    const unsigned long long sum = block_sum(mine, part);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void wt_exscan_kernel(const int *__restrict__ cnt, long long n, const unsigned long long *__restrict__ blockoff,
                                                        int *__restrict__ out) {
    __shared__ unsigned long long part[256];
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * SEED_ITEMS;
    unsigned long long mine = 0;
    for (int k = 0; k < SEED_ITEMS; k++) if (base + k < n) mine += (unsigned)cnt[base + k];
    unsigned long long pos = blockoff[blockIdx.x] + block_exclusive_scan(mine, part);
    for (int k = 0; k < SEED_ITEMS; k++) {
        const long long i = base + k;
        if (i >= n) break;
        out[i] = (int)pos;                                               // (the caller refuses totals above 2^31 - 1)
        pos += (unsigned)cnt[i];
    }
}

template <class T> __device__ __forceinline__ long long wt_lower_bound(const T *__restrict__ a, long long n, T v) {
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}
template <class T> __device__ __forceinline__ long long wt_upper_bound(const T *__restrict__ a, long long n, T v) {
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (a[mid] <= v) lo = mid + 1; else hi = mid; }
    return lo;
}

// ---- 1. occurrences --------------------------------------------------------------------------------------------------------
// the string symbol i belongs to: the last one that starts at or before i (empty strings in front of it share its start)
__device__ __forceinline__ int wt_string_of(const long long *__restrict__ start, int n_strings, long long i) {
    return (int)wt_upper_bound(start, (long long)n_strings, i) - 1;
}

// flag[i] = 1 where the last `wordlen` columns of i's own string are all letters (seeder.c:499-519)
__global__ __launch_bounds__(256) void wt_occ_flag_kernel(const uint8_t *__restrict__ sym, long long n, const long long *__restrict__ start,
                                                          int n_strings, int wordlen, int *__restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = wt_string_of(start, n_strings, i);
    bool ok = i - start[s] >= wordlen - 1;
    for (int w = 0; ok && w < wordlen; w++) ok = sym[i - w] != 0;
    flag[i] = ok;
}

// occurrence g: its code, its seed (pair, pos * pos_scale + pos_offset: seeder.c:540-545) and itself as the sort's payload
__global__ __launch_bounds__(256) void wt_occ_fill_kernel(const uint8_t *__restrict__ sym, long long n, const long long *__restrict__ start,
                                                          int n_strings, const c4gpu_word_source *__restrict__ src, int width, int wordlen,
                                                          const int *__restrict__ flag, const int *__restrict__ g_of,
                                                          unsigned long long *__restrict__ codes, c4gpu_seed_emit *__restrict__ seeds,
                                                          int *__restrict__ vals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int s = wt_string_of(start, n_strings, i), g = g_of[i];
    const int pos = (int)(i - start[s]) - wordlen + 1;
    unsigned long long code = 0;
    for (int w = 0; w < wordlen; w++) code = code * (unsigned)width + sym[i - wordlen + 1 + w];
    const c4gpu_word_source so = src[s];
    codes[g] = code;
    seeds[g] = c4gpu_seed_emit{so.pair, pos * so.pos_scale + so.pos_offset};
    vals[g] = g;
}

// ---- 2. seeded words: the runs of the sorted codes -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wt_head_flag_kernel(const unsigned long long *__restrict__ sc, long long n, int *__restrict__ head) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x < n) head[x] = x == 0 || sc[x - 1] != sc[x];
}

// seeded word u (code ascending): its code, where its run starts (w_start[n_seeded] = n_occ), and a mark at its first occurrence
__global__ __launch_bounds__(256) void wt_seeded_fill_kernel(const unsigned long long *__restrict__ sc, const int *__restrict__ so, long long n_occ,
                                                             const int *__restrict__ head, const int *__restrict__ u_of, int n_seeded,
                                                             unsigned long long *__restrict__ w_code, int *__restrict__ w_start,
                                                             int *__restrict__ first_flag) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= n_occ) return;
    if (x == 0) w_start[n_seeded] = (int)n_occ;
    if (!head[x]) return;
    const int u = u_of[x];
    w_code[u] = sc[x];
    w_start[u] = (int)x;
    first_flag[so[x]] = 1;
}

// by_rank[r] = the seeded word whose first occurrence is the r-th first occurrence
__global__ __launch_bounds__(256) void wt_rank_kernel(const int *__restrict__ so, const int *__restrict__ w_start, const int *__restrict__ rank_of_g,
                                                      int n_seeded, int *__restrict__ by_rank) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u < n_seeded) by_rank[rank_of_g[so[w_start[u]]]] = u;
}

// ---- 3. neighbourhoods -----------------------------------------------------------------------------------------------------
// One wave per seeded word W, wave j the word of rank n_seeded - 1 - j.  LDS: the rows s[W_k][.] of the score table, the depth
// thresholds (wordhood.c:207-216: thr[L-1] = T, thr[i] = thr[i+1] - s[W_{i+1}][W_{i+1}]; a prefix of length d+1 must score
// >= thr[d]), and per lane the walk's letter and the code in front of it at every depth.  The lanes take the two-letter prefixes
// round-robin and walk the rest depth first exactly as WordHood_traverse_word prunes (wordhood.c:277-299): a node whose partial
// score is below its depth's threshold is left, whatever the letters behind it could add.  FILL = false: lane_io[j * 64 + lane]
// = the words this lane reaches; FILL = true: lane_io holds their prefix sum and the same walk writes (code, j) from there.
__host__ __device__ inline size_t wt_hood_lds(int width, int L) {
    return (size_t)L * 64 * 8 + ((size_t)L * width + 2 * (size_t)L) * 4 + (size_t)L * 64;
}

template <bool FILL>
__global__ __launch_bounds__(64) void wt_hood_kernel(const unsigned long long *__restrict__ w_code, const int *__restrict__ by_rank, int n_seeded,
                                                     int width, int L, const int *__restrict__ scores, int threshold, int use_dropoff,
                                                     int *__restrict__ lane_io, unsigned long long *__restrict__ link_code,
                                                     int *__restrict__ link_j) {
    extern __shared__ unsigned long long wt_lds[];
    unsigned long long *code_at = wt_lds;                               // [d * 64 + lane]: the code in front of depth d
    int *row = (int *)(code_at + (size_t)L * 64);                       // [k * width + c] = s[W_k][c]
    int *thr = row + (size_t)L * width;                                 // [k]
    int *wl = thr + L;                                                  // [k] = W_k
    uint8_t *let = (uint8_t *)(wl + L);                                 // [d * 64 + lane]: the letter the walk holds at depth d
    const int j = blockIdx.x, lane = threadIdx.x;
    const unsigned long long wcode = w_code[by_rank[n_seeded - 1 - j]];
    if (lane == 0) {
        unsigned long long c = wcode;
        for (int k = L - 1; k >= 0; k--) { wl[k] = (int)(c % (unsigned)width); c /= (unsigned)width; }
    }
    __syncthreads();
    for (int x = lane; x < L * width; x += 64) row[x] = scores[wl[x / width] * width + x % width];
    __syncthreads();
    if (lane == 0) {
        int t = threshold;
        if (use_dropoff) { t = -threshold; for (int k = 0; k < L; k++) t += row[k * width + wl[k]]; }      // wordhood.c:331-337
        thr[L - 1] = t;
        for (int k = L - 2; k >= 0; k--) thr[k] = thr[k + 1] - row[(k + 1) * width + wl[k + 1]];
    }
    __syncthreads();
    const int A = width - 1, P = L < 2 ? 1 : 2, n_pref = P == 1 ? A : A * A;
    long long out = FILL ? lane_io[(size_t)j * 64 + lane] : 0;
    int count = 0;
    auto leaf = [&](unsigned long long n) {
        if (n == wcode) return;                                         // the word itself is not a neighbour (seeder.c:470)
        if (FILL) { link_code[out] = n; link_j[out] = j; out++; }
        count++;
    };
    for (int p = lane; p < n_pref; p += 64) {
        const int a = P == 1 ? p + 1 : p / A + 1;
        int sc = row[a];
        if (sc < thr[0]) continue;
        unsigned long long code = (unsigned)a;
        if (P == 2) {
            const int b = p % A + 1;
            sc += row[width + b];
            if (sc < thr[1]) continue;
            code = code * (unsigned)width + (unsigned)b;
        }
        if (L == P) { leaf(code); continue; }
        int d = P;
        let[d * 64 + lane] = 0;
        for (;;) {
            const int c = let[d * 64 + lane] + 1;
            if (c >= width) {                                           // this depth is through: back to the letter above
                if (d == P) break;
                d--;
                sc -= row[d * width + let[d * 64 + lane]];
                code = code_at[d * 64 + lane];
                continue;
            }
            let[d * 64 + lane] = (uint8_t)c;
            const int s2 = sc + row[d * width + c];
            if (s2 < thr[d]) continue;
            if (d == L - 1) { leaf(code * (unsigned)width + (unsigned)c); continue; }
            code_at[d * 64 + lane] = code;
            sc = s2;
            code = code * (unsigned)width + (unsigned)c;
            d++;
            let[d * 64 + lane] = 0;
        }
    }
    if (!FILL) lane_io[(size_t)j * 64 + lane] = count;
}

// ---- 5. the word list ------------------------------------------------------------------------------------------------------
// new_flag[y] = 1 at the head of a run of link codes that no query spells (a word with neighbour lists only)
__global__ __launch_bounds__(256) void wt_link_flag_kernel(const unsigned long long *__restrict__ lc, long long n_links,
                                                           const unsigned long long *__restrict__ w_code, int n_seeded, int *__restrict__ new_flag) {
    const long long y = (long long)blockIdx.x * 256 + threadIdx.x;
    if (y >= n_links) return;
    int nf = 0;
    if (y == 0 || lc[y - 1] != lc[y]) {
        const long long lb = wt_lower_bound(w_code, (long long)n_seeded, lc[y]);
        nf = !(lb < n_seeded && w_code[lb] == lc[y]);
    }
    new_flag[y] = nf;
}

// word k (code ascending over both kinds): its code, its seeded word (or -1) and its run of links [y0, y1)
__global__ __launch_bounds__(256) void wt_place_seeded_kernel(const unsigned long long *__restrict__ w_code, int n_seeded,
                                                              const unsigned long long *__restrict__ lc, long long n_links,
                                                              const int *__restrict__ new_pre, unsigned long long *__restrict__ word_code,
                                                              int *__restrict__ word_u, int *__restrict__ word_y0, int *__restrict__ word_y1) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n_seeded) return;
    const unsigned long long code = w_code[u];
    const long long y0 = wt_lower_bound(lc, n_links, code), y1 = wt_upper_bound(lc, n_links, code);
    const int k = u + (n_links ? new_pre[y0] : 0);                      // the new codes below this one
    word_code[k] = code; word_u[k] = u; word_y0[k] = (int)y0; word_y1[k] = (int)y1;
}

__global__ __launch_bounds__(256) void wt_place_new_kernel(const unsigned long long *__restrict__ lc, long long n_links, const int *__restrict__ new_flag,
                                                           const int *__restrict__ new_pre, const unsigned long long *__restrict__ w_code, int n_seeded,
                                                           unsigned long long *__restrict__ word_code, int *__restrict__ word_u,
                                                           int *__restrict__ word_y0, int *__restrict__ word_y1) {
    const long long y = (long long)blockIdx.x * 256 + threadIdx.x;
    if (y >= n_links || !new_flag[y]) return;
    const unsigned long long code = lc[y];
    const int k = new_pre[y] + (int)wt_lower_bound(w_code, (long long)n_seeded, code);
    word_code[k] = code; word_u[k] = -1; word_y0[k] = (int)y; word_y1[k] = (int)wt_upper_bound(lc, n_links, code);
}

// the length of word k's emission list: own(N), then own(W) of every link (seeder.c:676-692)
__global__ __launch_bounds__(256) void wt_word_count_kernel(int n_words, const int *__restrict__ word_u, const int *__restrict__ word_y0,
                                                            const int *__restrict__ word_y1, const int *__restrict__ w_start,
                                                            const int *__restrict__ lj, const int *__restrict__ by_rank, int n_seeded,
                                                            int *__restrict__ word_cnt, unsigned long long *__restrict__ too_many) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_words) return;
    const int u = word_u[k];
    long long c = u >= 0 ? w_start[u + 1] - w_start[u] : 0;
    for (int y = word_y0[k]; y < word_y1[k]; y++) {
        const int w = by_rank[n_seeded - 1 - lj[y]];
        c += w_start[w + 1] - w_start[w];
    }
    if (c > 0x7fffffffLL) { *too_many = 1; c = 0x7fffffffLL; }
    word_cnt[k] = (int)c;
}

// one wave per word: its lists to their places.  A run of the sorted occurrences is g ascending; a seed list is g descending
__global__ __launch_bounds__(256) void wt_emit_fill_kernel(int n_words, const int *__restrict__ word_u, const int *__restrict__ word_y0,
                                                           const int *__restrict__ word_y1, const int *__restrict__ emit_first,
                                                           const int *__restrict__ w_start, const int *__restrict__ so,
                                                           const c4gpu_seed_emit *__restrict__ occ_seed, const int *__restrict__ lj,
                                                           const int *__restrict__ by_rank, int n_seeded, c4gpu_seed_emit *__restrict__ emits) {
    const long long k = (long long)blockIdx.x * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (k >= n_words) return;
    long long off = emit_first[k];
    auto copy = [&](int w) {
        const int x0 = w_start[w], len = w_start[w + 1] - x0;
        for (int t = lane; t < len; t += 64) emits[off + t] = occ_seed[so[x0 + len - 1 - t]];
        off += len;
    };
    if (word_u[k] >= 0) copy(word_u[k]);
    for (int y = word_y0[k]; y < word_y1[k]; y++) copy(by_rank[n_seeded - 1 - lj[y]]);
}

// the slots of seed_count_kernel's hash.  No word has code 0 (its letters are columns >= 1), so 0 marks a free slot
__global__ __launch_bounds__(256) void wt_slot_insert_kernel(int n_words, const unsigned long long *__restrict__ word_code,
                                                             const int *__restrict__ emit_first, WordSlot *slots, unsigned mask) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_words) return;
    const unsigned long long code = word_code[k];
    unsigned h = (unsigned)word_hash(code) & mask;
    while (atomicCAS(&slots[h].code, 0ull, code) != 0ull) h = (h + 1) & mask;
    slots[h].first = emit_first[k];
    slots[h].count = emit_first[k + 1] - emit_first[k];
}

struct WtWork {
    DevBuf<long long> start;
    DevBuf<c4gpu_word_source> src;
    DevBuf<int> scores, flag, g_of, head, u_of, first_flag, rank_of_g, w_start, by_rank, lane_cnt, lane_off, new_flag, new_pre,
                word_u, word_y0, word_y1, word_cnt, vals[2];
    DevBuf<unsigned long long> keys[2], w_code, blocks, hist, tot;
    DevBuf<c4gpu_seed_emit> occ_seed;
};

inline int wt_grid(long long n) { return (int)((n + 255) / 256); }

// out[i] = the sum of cnt[0 .. i), tot[slot] = the sum of all n
int wt_scan(WtWork &w, hipStream_t s, const int *cnt, long long n, int *out, int slot) {
    const int nb = seed_count_blocks(n);
    if (w.blocks.alloc((size_t)nb)) return -1;
    hipLaunchKernelGGL(wt_blocksum_kernel, dim3(nb), dim3(256), 0, s, cnt, n, w.blocks.p);
    hipLaunchKernelGGL(seed_blockscan_kernel, dim3(1), dim3(1024), 0, s, w.blocks.p, nb, w.tot.p + slot);
    hipLaunchKernelGGL(wt_exscan_kernel, dim3(nb), dim3(256), 0, s, cnt, n, (const unsigned long long *)w.blocks.p, out);
    return 0;
}

int wt_read(WtWork &w, hipStream_t s, int slot, unsigned long long *v) {
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(v, w.tot.p + slot, sizeof *v, hipMemcpyDeviceToHost, s));
    HIP_OK(c4_stream_sync(s));
    return 0;
}

// the stable radix sort of c4_seed_dev.inc over 64-bit keys below `span`; returns which of the two buffers holds the result
int wt_sort(WtWork &w, hipStream_t s, DevBuf<unsigned long long> *keys, DevBuf<int> *vals, long long n, double span, int *cur_out) {
    const int n_tiles = (int)((n + SEED_SORT_TILE - 1) / SEED_SORT_TILE);
    if (w.hist.alloc((size_t)256 * n_tiles) || keys[1].alloc((size_t)n) || vals[1].alloc((size_t)n)) return -1;
    int passes = 1, cur = 0;
    for (double v = 256; v < span; v *= 256) passes++;
    for (int p = 0; p < passes; p++, cur ^= 1) {
        hipLaunchKernelGGL(seed_sort_hist_kernel<unsigned long long>, dim3(n_tiles), dim3(64), 0, s, keys[cur].p, n, 8 * p, n_tiles, w.hist.p);
        hipLaunchKernelGGL(seed_blockscan_kernel, dim3(1), dim3(1024), 0, s, w.hist.p, 256 * n_tiles, w.tot.p + 7);
        hipLaunchKernelGGL(seed_sort_scatter_kernel<unsigned long long>, dim3(n_tiles), dim3(64), 0, s, keys[cur].p, vals[cur].p, n, 8 * p,
                           n_tiles, w.hist.p, keys[cur ^ 1].p, vals[cur ^ 1].p);
    }
    *cur_out = cur;
    return 0;
}

int wt_fail(const std::string &what) { c4h::set_error("c4gpu_wordtab_build: " + what); return -1; }

int wt_build(c4gpu_ctx *ctx, c4gpu_wordtab *t, const uint8_t *const *symbols, const int32_t *n_symbols, const c4gpu_word_source *src,
             int n_strings, const int32_t *scores, int threshold, int use_dropoff, c4gpu_wordtab_build_stats *st) {
    const int width = t->width, L = t->wordlen;
    hipStream_t s = ctx->stream;
    WtWork w;
    // the strings behind each other
    std::vector<long long> start((size_t)n_strings + 1, 0);
    for (int k = 0; k < n_strings; k++) start[k + 1] = start[k] + n_symbols[k];
    const long long n_sym = start[n_strings];
    unsigned size = 16;
    long long n_occ = 0, n_seeded = 0, n_links = 0, n_words = 0, n_emits = 0;
    unsigned long long v = 0;
    if (w.tot.alloc(8)) return -1;
    HIP_OK(hipMemsetAsync(w.tot.p, 0, 8 * sizeof(unsigned long long), s));
    if (n_sym > 0) {
        std::vector<uint8_t> hsym((size_t)n_sym);
        for (int k = 0; k < n_strings; k++) if (n_symbols[k]) memcpy(hsym.data() + start[k], symbols[k], (size_t)n_symbols[k]);
        if (t->d_sym.upload(hsym.data(), (size_t)n_sym, s) || w.start.upload(start.data(), start.size(), s) ||
            w.src.upload(src, (size_t)n_strings, s) || w.flag.alloc((size_t)n_sym) || w.g_of.alloc((size_t)n_sym)) return -1;
        hipLaunchKernelGGL(wt_occ_flag_kernel, dim3(wt_grid(n_sym)), dim3(256), 0, s, t->d_sym.p, n_sym, w.start.p, n_strings, L, w.flag.p);
        if (wt_scan(w, s, w.flag.p, n_sym, w.g_of.p, 0) || wt_read(w, s, 0, &v)) return -1;     // (the sync also covers `hsym`)
        n_occ = (long long)v;
    }
    if (n_occ > 0) {
        // 1., 2.
        double span = 1;
        for (int k = 0; k < L; k++) span *= width;
        int cur = 0;
        if (w.keys[0].alloc((size_t)n_occ) || w.vals[0].alloc((size_t)n_occ) || w.occ_seed.alloc((size_t)n_occ) || w.head.alloc((size_t)n_occ) ||
            w.u_of.alloc((size_t)n_occ) || w.first_flag.alloc((size_t)n_occ) || w.rank_of_g.alloc((size_t)n_occ)) return -1;
        hipLaunchKernelGGL(wt_occ_fill_kernel, dim3(wt_grid(n_sym)), dim3(256), 0, s, t->d_sym.p, n_sym, w.start.p, n_strings, w.src.p, width, L,
                           w.flag.p, w.g_of.p, w.keys[0].p, w.occ_seed.p, w.vals[0].p);
        if (wt_sort(w, s, w.keys, w.vals, n_occ, span, &cur)) return -1;
        const unsigned long long *sc = w.keys[cur].p;
        const int *so = w.vals[cur].p;
        hipLaunchKernelGGL(wt_head_flag_kernel, dim3(wt_grid(n_occ)), dim3(256), 0, s, sc, n_occ, w.head.p);
        if (wt_scan(w, s, w.head.p, n_occ, w.u_of.p, 1) || wt_read(w, s, 1, &v)) return -1;
        n_seeded = (long long)v;
        if (w.w_code.alloc((size_t)n_seeded) || w.w_start.alloc((size_t)n_seeded + 1) || w.by_rank.alloc((size_t)n_seeded)) return -1;
        HIP_OK(hipMemsetAsync(w.first_flag.p, 0, (size_t)n_occ * sizeof(int), s));
        hipLaunchKernelGGL(wt_seeded_fill_kernel, dim3(wt_grid(n_occ)), dim3(256), 0, s, sc, so, n_occ, w.head.p, w.u_of.p, (int)n_seeded,
                           w.w_code.p, w.w_start.p, w.first_flag.p);
        if (wt_scan(w, s, w.first_flag.p, n_occ, w.rank_of_g.p, 2)) return -1;
        hipLaunchKernelGGL(wt_rank_kernel, dim3(wt_grid(n_seeded)), dim3(256), 0, s, so, w.w_start.p, w.rank_of_g.p, (int)n_seeded, w.by_rank.p);
        // 3., 4.  (the sorted occurrences stay where they are: the links get buffers of their own)
        DevBuf<unsigned long long> lkeys[2];
        DevBuf<int> lvals[2];
        const unsigned long long *lc = nullptr;
        const int *lj = nullptr;
        if (scores) {
            const size_t lds = wt_hood_lds(width, L);
            if (w.scores.upload(scores, (size_t)width * width, s) || w.lane_cnt.alloc((size_t)n_seeded * 64) ||
                w.lane_off.alloc((size_t)n_seeded * 64)) return -1;
            hipLaunchKernelGGL(wt_hood_kernel<false>, dim3((unsigned)n_seeded), dim3(64), lds, s, w.w_code.p, w.by_rank.p, (int)n_seeded, width, L,
                               w.scores.p, threshold, use_dropoff, w.lane_cnt.p, (unsigned long long *)nullptr, (int *)nullptr);
            if (wt_scan(w, s, w.lane_cnt.p, n_seeded * 64, w.lane_off.p, 3) || wt_read(w, s, 3, &v)) return -1;
            if (v > 0x7fffffffULL) return wt_fail("more than 2^31 - 1 neighbour links");
            n_links = (long long)v;
        }
        if (n_links > 0) {
            if (lkeys[0].alloc((size_t)n_links) || lvals[0].alloc((size_t)n_links)) return -1;
            hipLaunchKernelGGL(wt_hood_kernel<true>, dim3((unsigned)n_seeded), dim3(64), wt_hood_lds(width, L), s, w.w_code.p, w.by_rank.p,
                               (int)n_seeded, width, L, w.scores.p, threshold, use_dropoff, w.lane_off.p, lkeys[0].p, lvals[0].p);
            int lcur = 0;
            if (wt_sort(w, s, lkeys, lvals, n_links, span, &lcur)) return -1;
            lc = lkeys[lcur].p; lj = lvals[lcur].p;
        }
        // 5.
        long long n_new = 0;
        if (n_links > 0) {
            if (w.new_flag.alloc((size_t)n_links + 1) || w.new_pre.alloc((size_t)n_links + 1)) return -1;
            HIP_OK(hipMemsetAsync(w.new_flag.p + n_links, 0, sizeof(int), s));
            hipLaunchKernelGGL(wt_link_flag_kernel, dim3(wt_grid(n_links)), dim3(256), 0, s, lc, n_links, w.w_code.p, (int)n_seeded, w.new_flag.p);
            if (wt_scan(w, s, w.new_flag.p, n_links + 1, w.new_pre.p, 4) || wt_read(w, s, 4, &v)) return -1;
            n_new = (long long)v;
        }
        n_words = n_seeded + n_new;
        if (n_words > (1LL << 30)) return wt_fail("more than 2^30 words");
        if (t->d_codes.alloc((size_t)n_words) || t->d_emit_first.alloc((size_t)n_words + 1) || w.word_u.alloc((size_t)n_words) ||
            w.word_y0.alloc((size_t)n_words) || w.word_y1.alloc((size_t)n_words) || w.word_cnt.alloc((size_t)n_words + 1)) return -1;
        hipLaunchKernelGGL(wt_place_seeded_kernel, dim3(wt_grid(n_seeded)), dim3(256), 0, s, w.w_code.p, (int)n_seeded, lc, n_links, w.new_pre.p,
                           t->d_codes.p, w.word_u.p, w.word_y0.p, w.word_y1.p);
        if (n_links > 0)
            hipLaunchKernelGGL(wt_place_new_kernel, dim3(wt_grid(n_links)), dim3(256), 0, s, lc, n_links, w.new_flag.p, w.new_pre.p, w.w_code.p,
                               (int)n_seeded, t->d_codes.p, w.word_u.p, w.word_y0.p, w.word_y1.p);
        HIP_OK(hipMemsetAsync(w.word_cnt.p + n_words, 0, sizeof(int), s));
        hipLaunchKernelGGL(wt_word_count_kernel, dim3(wt_grid(n_words)), dim3(256), 0, s, (int)n_words, w.word_u.p, w.word_y0.p, w.word_y1.p,
                           w.w_start.p, lj, w.by_rank.p, (int)n_seeded, w.word_cnt.p, w.tot.p + 6);
        if (wt_scan(w, s, w.word_cnt.p, n_words + 1, t->d_emit_first.p, 5) || wt_read(w, s, 5, &v)) return -1;
        unsigned long long too_many = 0;
        if (wt_read(w, s, 6, &too_many)) return -1;
        if (too_many || v > 0x7fffffffULL) return wt_fail("more than 2^31 - 1 emissions");
        n_emits = (long long)v;
        while (size < 2u * (unsigned)n_words) size <<= 1;
        if (t->d_emits.alloc((size_t)n_emits) || t->slots.alloc(size)) return -1;
        HIP_OK(hipMemsetAsync(t->slots.p, 0, (size_t)size * sizeof(WordSlot), s));
        hipLaunchKernelGGL(wt_emit_fill_kernel, dim3((unsigned)((n_words + 3) / 4)), dim3(256), 0, s, (int)n_words, w.word_u.p, w.word_y0.p,
                           w.word_y1.p, t->d_emit_first.p, w.w_start.p, so, w.occ_seed.p, lj, w.by_rank.p, (int)n_seeded, t->d_emits.p);
        hipLaunchKernelGGL(wt_slot_insert_kernel, dim3(wt_grid(n_words)), dim3(256), 0, s, (int)n_words, t->d_codes.p, t->d_emit_first.p,
                           t->slots.p, size - 1);
        HIP_OK(hipGetLastError());
        HIP_OK(c4_stream_sync(s));                                      // (the work buffers go away with `w`)
    } else {
        if (t->slots.alloc(size) || t->d_emits.alloc(1)) return -1;
        HIP_OK(hipMemsetAsync(t->slots.p, 0, (size_t)size * sizeof(WordSlot), s));
        HIP_OK(c4_stream_sync(s));
    }
    t->mask = size - 1;
    t->n_words = (int)n_words;
    t->n_emissions = (int)n_emits;
    t->emits_set = true;
    t->emit_max_pair = -1;
    // (c4gpu_seed_extend wants every pair an emission names inside its `pairs`: here, every source's, unless nothing is emitted)
    for (int k = 0; n_emits && k < n_strings; k++) t->emit_max_pair = std::max(t->emit_max_pair, src[k].pair);
    t->built = true;
    if (st) { st->n_occurrences = n_occ; st->n_seeded_words = n_seeded; st->n_links = n_links; st->n_words = n_words; st->n_emits = n_emits; }
    return 0;
}

}  // namespace

extern "C" c4gpu_wordtab *c4gpu_wordtab_build(c4gpu_ctx *ctx, int32_t width, int32_t wordlen, const uint8_t *const *symbols,
                                              const int32_t *n_symbols, const c4gpu_word_source *src, int32_t n_strings,
                                              const int32_t *scores, int32_t threshold, int32_t use_dropoff,
                                              c4gpu_wordtab_build_stats *stats) {
    if (stats) *stats = c4gpu_wordtab_build_stats{0, 0, 0, 0, 0, 0.0};
    // everything that is refused is refused here, before the device is touched
    if (width < 2 || width > 255 || wordlen < 1 || wordlen > 32 || n_strings < 0) { wt_fail("bad shape"); return nullptr; }
    double span = 1;
    for (int k = 0; k < wordlen; k++) span *= width;
    if (span >= 9.2e18) { wt_fail("width^wordlen does not fit 63 bits"); return nullptr; }
    long long total = 0;
    for (int k = 0; k < n_strings; k++) {
        if (n_symbols[k] < 0) { wt_fail("a string of negative length"); return nullptr; }
        if (src[k].pair < 0 || src[k].pos_scale < 1 || src[k].pos_offset < 0) {
            wt_fail("a source with a negative pair or offset, or a scale below 1");
            return nullptr;
        }
        if ((long long)n_symbols[k] * src[k].pos_scale + src[k].pos_offset > 0x7fffffffLL) { wt_fail("a query position above 2^31 - 1"); return nullptr; }
        total += n_symbols[k];
    }
    if (total > 0x7fffffffLL) { wt_fail("more than 2^31 - 1 symbols"); return nullptr; }
    if (scores) {
        for (int k = 0; k < width * width; k++)
            if (scores[k] > (1 << 20) || scores[k] < -(1 << 20)) { wt_fail("a score beyond +-2^20"); return nullptr; }
        if (threshold > (1 << 28) || threshold < -(1 << 28)) { wt_fail("a threshold beyond +-2^28"); return nullptr; }
    }
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return nullptr; }
    try {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<c4gpu_wordtab> t(new c4gpu_wordtab);
        t->ctx = ctx; t->width = width; t->wordlen = wordlen; t->n_words = 0;
        if (wt_build(ctx, t.get(), symbols, n_symbols, src, n_strings, scores, threshold, use_dropoff ? 1 : 0, stats)) return nullptr;
        if (stats) stats->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return t.release();
    } catch (const std::exception &e) {
        c4h::set_error(std::string("c4gpu_wordtab_build: ") + e.what());
        return nullptr;
    }
}

extern "C" int c4gpu_wordtab_export(c4gpu_ctx *ctx, c4gpu_wordtab *t, uint64_t *codes, int32_t *emit_first, int64_t cap_words,
                                    c4gpu_seed_emit *emits, int64_t cap_emits, int64_t *n_words, int64_t *n_emits) {
    if (hipSetDevice(ctx->device) != hipSuccess) { c4h::set_error("hipSetDevice failed"); return -1; }
    if (!t->emits_set) { c4h::set_error("c4gpu_wordtab_export: no emissions set (c4gpu_wordtab_set_emissions)"); return -1; }
    if (!t->built)
        for (int k = 1; k < t->n_words; k++)
            if (t->h_codes[k - 1] >= t->h_codes[k]) { c4h::set_error("c4gpu_wordtab_export: the table's words were not given by code ascending"); return -1; }
    *n_words = t->n_words; *n_emits = t->n_emissions;
    if (t->n_words > cap_words || t->n_emissions > cap_emits) return 0;     // the caller comes back with room for all of them
    emit_first[0] = 0;
    if (!t->n_words) return 0;
    hipStream_t s = ctx->stream;
    if (t->built) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "codes are downloaded in place");
        if (t->d_codes.download(reinterpret_cast<unsigned long long *>(codes), (size_t)t->n_words, s) ||
            t->d_emit_first.download(emit_first, (size_t)t->n_words + 1, s)) return -1;
    } else {
        memcpy(codes, t->h_codes.data(), (size_t)t->n_words * sizeof(uint64_t));
        memcpy(emit_first, t->h_first.data(), ((size_t)t->n_words + 1) * sizeof(int32_t));
    }
    if (t->n_emissions && t->d_emits.download(emits, (size_t)t->n_emissions, s)) return -1;
    HIP_OK(c4_stream_sync(s));
    return 0;
}
