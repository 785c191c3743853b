// c4_engine_staging.inc -- part of c4_engine.hip (one translation unit; included there, in this order): what a batch needs before its first DP cell: model families, sequence preparation kernels (residue coding, codon tables, splice arrays), the device side of the reduced-space route, ResidentSeqs.
// ---- which compiled family does a flattened model belong to? ----------------------------------------------
template <class M>
bool model_matches(const c4gpu_model &m) {
    if (m.n_states != M::NS || m.n_transitions != M::NT || m.n_calcs != M::NC || m.n_shadows != M::NSH) return false;
    if (m.start_state != M::START || m.end_state != M::END || m.total_shadow_designations != M::NDES) return false;
    for (int k = 0; k < M::NT; k++) {
        const c4gpu_transition &t = m.transitions[k];
        const TrDesc &d = M::tr[k];
        if (t.input != d.in || t.output != d.out || t.advance_query != d.aq || t.advance_target != d.at ||
            t.calc != d.calc || t.label != d.label || t.dst_shadow_mask != d.dst_shadow_mask) return false;
    }
    for (int c = 0; c < M::NC; c++) {
        const int kind = m.calcs[c].kind, dk = M::calc[c].kind;
        const bool both_11 = (kind == C4GPU_CALC_MATCH_DNA || kind == C4GPU_CALC_MATCH_PROTEIN) &&
                             (dk == C4GPU_CALC_MATCH_DNA || dk == C4GPU_CALC_MATCH_PROTEIN);
        if (!both_11 && kind != dk) return false;
        if (kind >= C4GPU_CALC_SPLICE_PRE && m.calcs[c].param != M::calc[c].param) return false;
        if (m.calcs[c].protect != M::calc[c].protect) return false;
    }
    for (int s = 0; s < M::NSH; s++) {
        if (m.shadows[s].designation != M::sh[s].designation || m.shadows[s].on_target != M::sh[s].on_target ||
            m.shadows[s].src_state_mask != M::sh[s].src_state_mask ||
            m.shadows[s].dst_transition_mask != M::sh[s].dst_transition_mask) return false;
    }
    return true;
}

int model_family(const c4gpu_model &m) {
    if (model_matches<UngappedDesc>(m)) return FAM_UNGAPPED;
    if (model_matches<AffineDesc>(m)) return FAM_AFFINE;
    if (model_matches<Est2GenomeDesc>(m)) return FAM_EST2GENOME;
    if (model_matches<UngappedP2DDesc>(m)) return FAM_UNGAPPED_P2D;
    if (model_matches<Protein2DnaDesc>(m)) return FAM_PROTEIN2DNA;
    if (model_matches<Protein2GenomeDesc>(m)) return FAM_PROTEIN2GENOME;
    if (model_matches<AffineStartDesc>(m)) return FAM_AFFINE_START;
    if (model_matches<AffineEndDesc>(m)) return FAM_AFFINE_END;
    if (model_matches<AffineJoinDesc>(m)) return FAM_AFFINE_JOIN;
    if (model_matches<Est2GenomeFwdStartDesc>(m)) return FAM_EST2GENOME_FWD_START;
    if (model_matches<Est2GenomeFwdEndDesc>(m)) return FAM_EST2GENOME_FWD_END;
    if (model_matches<Est2GenomeFwdJoinDesc>(m)) return FAM_EST2GENOME_FWD_JOIN;
    if (model_matches<Est2GenomeRevStartDesc>(m)) return FAM_EST2GENOME_REV_START;
    if (model_matches<Est2GenomeRevEndDesc>(m)) return FAM_EST2GENOME_REV_END;
    if (model_matches<Est2GenomeRevJoinDesc>(m)) return FAM_EST2GENOME_REV_JOIN;
    if (model_matches<Protein2DnaStartDesc>(m)) return FAM_PROTEIN2DNA_START;
    if (model_matches<Protein2DnaEndDesc>(m)) return FAM_PROTEIN2DNA_END;
    if (model_matches<Protein2DnaJoinDesc>(m)) return FAM_PROTEIN2DNA_JOIN;
    if (model_matches<Protein2GenomeStartDesc>(m)) return FAM_PROTEIN2GENOME_START;
    if (model_matches<Protein2GenomeEndDesc>(m)) return FAM_PROTEIN2GENOME_END;
    if (model_matches<Protein2GenomeJoinDesc>(m)) return FAM_PROTEIN2GENOME_JOIN;
    if (model_matches<Est2GenomeFwdSpanSrcDesc>(m)) return FAM_EST2GENOME_FWD_SPAN_SRC;
    if (model_matches<Est2GenomeFwdSpanDstDesc>(m)) return FAM_EST2GENOME_FWD_SPAN_DST;
    if (model_matches<Est2GenomeRevSpanSrcDesc>(m)) return FAM_EST2GENOME_REV_SPAN_SRC;
    if (model_matches<Est2GenomeRevSpanDstDesc>(m)) return FAM_EST2GENOME_REV_SPAN_DST;
    if (model_matches<Protein2GenomePhase0SpanSrcDesc>(m)) return FAM_PROTEIN2GENOME_PHASE0_SPAN_SRC;
    if (model_matches<Protein2GenomePhase0SpanDstDesc>(m)) return FAM_PROTEIN2GENOME_PHASE0_SPAN_DST;
    if (model_matches<Protein2GenomePhase1SpanSrcDesc>(m)) return FAM_PROTEIN2GENOME_PHASE1_SPAN_SRC;
    if (model_matches<Protein2GenomePhase1SpanDstDesc>(m)) return FAM_PROTEIN2GENOME_PHASE1_SPAN_DST;
    if (model_matches<Protein2GenomePhase2SpanSrcDesc>(m)) return FAM_PROTEIN2GENOME_PHASE2_SPAN_SRC;
    if (model_matches<Protein2GenomePhase2SpanDstDesc>(m)) return FAM_PROTEIN2GENOME_PHASE2_SPAN_DST;
    if (model_matches<NerDesc>(m)) return FAM_NER;
    if (model_matches<UngappedCodonDesc>(m)) return FAM_UNGAPPED_CODON;
    if (model_matches<Coding2CodingDesc>(m)) return FAM_CODING2CODING;
    if (model_matches<Coding2CodingStartDesc>(m)) return FAM_CODING2CODING_START;
    if (model_matches<Coding2CodingEndDesc>(m)) return FAM_CODING2CODING_END;
    if (model_matches<Coding2CodingJoinDesc>(m)) return FAM_CODING2CODING_JOIN;
    if (model_matches<Coding2GenomeDesc>(m)) return FAM_CODING2GENOME;
    if (model_matches<Coding2GenomeStartDesc>(m)) return FAM_CODING2GENOME_START;
    if (model_matches<Coding2GenomeEndDesc>(m)) return FAM_CODING2GENOME_END;
    if (model_matches<Coding2GenomeJoinDesc>(m)) return FAM_CODING2GENOME_JOIN;
    if (model_matches<Coding2GenomePhase0SpanSrcDesc>(m)) return FAM_CODING2GENOME_PHASE0_SPAN_SRC;
    if (model_matches<Coding2GenomePhase0SpanDstDesc>(m)) return FAM_CODING2GENOME_PHASE0_SPAN_DST;
    if (model_matches<Coding2GenomePhase1SpanSrcDesc>(m)) return FAM_CODING2GENOME_PHASE1_SPAN_SRC;
    if (model_matches<Coding2GenomePhase1SpanDstDesc>(m)) return FAM_CODING2GENOME_PHASE1_SPAN_DST;
    if (model_matches<Coding2GenomePhase2SpanSrcDesc>(m)) return FAM_CODING2GENOME_PHASE2_SPAN_SRC;
    if (model_matches<Coding2GenomePhase2SpanDstDesc>(m)) return FAM_CODING2GENOME_PHASE2_SPAN_DST;
    return -1;
}

static bool family_is_p2g_span(int fam) {
    return fam >= FAM_PROTEIN2GENOME_PHASE0_SPAN_SRC && fam <= FAM_PROTEIN2GENOME_PHASE2_SPAN_DST;
}
// coding2genome's six span models (one src / dst pair per intron phase), named one by one
static bool family_is_c2g_span(int fam) {
    return fam == FAM_CODING2GENOME_PHASE0_SPAN_SRC || fam == FAM_CODING2GENOME_PHASE0_SPAN_DST ||
           fam == FAM_CODING2GENOME_PHASE1_SPAN_SRC || fam == FAM_CODING2GENOME_PHASE1_SPAN_DST ||
           fam == FAM_CODING2GENOME_PHASE2_SPAN_SRC || fam == FAM_CODING2GENOME_PHASE2_SPAN_DST;
}
// coding2genome and BSDP's nine derived models of it: codon families (the query is translated per position) that are splice and
// phase families too (forward splice arrays, base masks, intron length limits)
bool family_is_coding2genome(int fam) {
    return fam == FAM_CODING2GENOME || fam == FAM_CODING2GENOME_START || fam == FAM_CODING2GENOME_END ||
           fam == FAM_CODING2GENOME_JOIN || family_is_c2g_span(fam);
}
// coding2coding and its three derived models
bool family_is_coding2coding(int fam) {
    return fam == FAM_CODING2CODING || fam == FAM_CODING2CODING_START || fam == FAM_CODING2CODING_END || fam == FAM_CODING2CODING_JOIN;
}
// both sequences translated (Match_3_3): the query array holds codon row codes too.  The derived models of coding2coding
// included: an engine of theirs on a coding2coding batch reads the batch's translated query codes (c4gpu_batch_viterbi_model)
// coding2genome is both a codon family and, below, an intron family: its batch gets codon row codes on both axes AND the forward
// splice arrays, the base masks and the intron length limits
bool family_is_codon(int fam) {
    return fam == FAM_UNGAPPED_CODON || (fam >= FAM_CODING2CODING && fam <= FAM_CODING2CODING_JOIN) || family_is_coding2genome(fam);
}
bool family_is_p2d(int fam) {
    return fam == FAM_UNGAPPED_P2D || fam == FAM_PROTEIN2DNA || fam == FAM_PROTEIN2GENOME ||
           (fam >= FAM_PROTEIN2DNA_START && fam <= FAM_PROTEIN2GENOME_JOIN) || family_is_p2g_span(fam) ||
           family_is_codon(fam);
}
bool family_has_splice(int fam) {
    return fam == FAM_EST2GENOME || fam == FAM_PROTEIN2GENOME || (fam >= FAM_EST2GENOME_FWD_START && fam <= FAM_EST2GENOME_REV_JOIN) ||
           (fam >= FAM_PROTEIN2GENOME_START && fam <= FAM_PROTEIN2GENOME_JOIN) ||
           (fam >= FAM_EST2GENOME_FWD_SPAN_SRC && fam <= FAM_EST2GENOME_REV_SPAN_DST) || family_is_p2g_span(fam) ||
           family_is_coding2genome(fam);
}
bool family_has_phase(int fam) {
    return fam == FAM_PROTEIN2GENOME || (fam >= FAM_PROTEIN2GENOME_START && fam <= FAM_PROTEIN2GENOME_JOIN) ||
           family_is_p2g_span(fam) || family_is_coding2genome(fam);
}

// ---- sequence preparation kernels -------------------------------------------------------------------------
struct PrepTables {
    uint8_t submat_index[256];
    uint8_t nt2d[256];
    uint8_t trans[4096];
    uint8_t aa[40];
};

// residue bytes -> substitution matrix row (Submat_lookup's index step, submat.h:54-56)
// (codes, when given: the set of rows that occur, one bit each -- what the staged packed score pass sizes its query profile by)
__global__ void encode_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long n,
                              const PrepTables *__restrict__ tab, int *bad, int *codes = nullptr) {
    int seen = 0;
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < n; x += (long long)gridDim.x * blockDim.x) {
        const uint8_t c = tab->submat_index[in[x]];
        if (c >= 24) atomicExch(bad, 1);
        out[x] = c >= 24 ? 0 : c;
        seen |= 1 << (c >= 24 ? 0 : c);
    }
    if (codes) {
        for (int off = 32; off > 0; off >>= 1) seen |= __shfl_xor(seen, off);
        if ((threadIdx.x & 63) == 0 && seen) atomicOr(codes, seen);
    }
}

// the targets' row codes as DENSE indices (0 .. 7) into the batch's code table (tab[code] -> index): what the packed checkpoint
// pass and region windows index their query profiles by (Prof16, c4_ckpt16_kernel.h)
__global__ void dense_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long n, const uint8_t *__restrict__ tab) {
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < n; x += (long long)gridDim.x * blockDim.x) {
        const uint8_t d = tab[in[x]];
        out[x] = d < 8 ? d : 0;
    }
}

// protein2dna target: row of the residue encoded by the codon starting at each position
// (Translate_base, translate.h:73-76, then the submat index)
__global__ void codon_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const long long *off,
                             const int *len, int n_seqs, const PrepTables *__restrict__ tab, int *bad) {
  for (int pair = blockIdx.y; pair < n_seqs; pair += gridDim.y) {
    const uint8_t *s = in + off[pair];
    uint8_t *o = out + off[pair];
    const int n = len[pair];
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
        uint8_t code = 0;
        if (x + 2 < n) {
            const uint8_t aa = tab->aa[tab->trans[tab->nt2d[s[x]] | (tab->nt2d[s[x + 1]] << 4) | (tab->nt2d[s[x + 2]] << 8)]];
            code = tab->submat_index[aa];
            if (code >= 24) { atomicExch(bad, 2); code = 0; }
        }
        o[x] = code;
    }
  }
}

// split-codon calcs (phase.c:188-208) re-read bases around an intron: per position the 4-bit base masks
// (Translate nt2d, translate.h:40-50) of positions p, p-1, p-2, p-3
__global__ void tn4_kernel(const uint8_t *__restrict__ in, uint16_t *__restrict__ out, const long long *off,
                           const int *len, int n_seqs, const PrepTables *__restrict__ tab) {
  for (int pair = blockIdx.y; pair < n_seqs; pair += gridDim.y) {
    const uint8_t *s = in + off[pair];
    uint16_t *o = out + off[pair];
    const int n = len[pair];
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
        unsigned v = 0;
        for (int d = 0; d < 4; d++)
            if (x - d >= 0) v |= (unsigned)tab->nt2d[s[x - d]] << (4 * d);
        o[x] = (uint16_t)v;
    }
  }
}

// SplicePredictor_predict_array_int (splice.c:383-397): float accumulation left to right over the PSSM
// window clipped to the sequence (Splice_predict_position, splice.c:320-344), rounded half away from
// zero in double (SplicePredictor_round, splice.c:379-381).  Plain adds only: no contraction possible.
__global__ void splice_kernel(const uint8_t *__restrict__ seq, const long long *off, const int *len, int n_seqs,
                              const c4gpu_splice_model *__restrict__ models, int *__restrict__ out,
                              long long stride) {
  const int type = blockIdx.z;
  const c4gpu_splice_model *sp = &models[type];
  for (int pair = blockIdx.y; pair < n_seqs; pair += gridDim.y) {
    const uint8_t *s = seq + off[pair];
    const int n = len[pair];
    int *o = out + (long long)type * stride + off[pair];
    for (int pos = blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += gridDim.x * blockDim.x) {
        int seq_start = pos - sp->splice_after, model_start = 0, calc_length = sp->model_length;
        if (seq_start < 0) { model_start = -seq_start; seq_start = 0; calc_length -= model_start; }
        if (seq_start + calc_length > n) calc_length = n - seq_start;
        float score = 0.0f;
        for (int i = 0; i < calc_length; i++) score = score + sp->data[model_start + i][sp->index[s[seq_start + i]]];
        if (sp->gtag_only) {                    // Splice_predict_is_on_GTAG, splice.c:312-318 (past the end: the NUL)
            const int b1 = s[pos], b2 = pos + 1 < n ? s[pos + 1] : 0;
            const int u1 = (b1 >= 'a' && b1 <= 'z') ? b1 - 32 : b1, u2 = (b2 >= 'a' && b2 <= 'z') ? b2 - 32 : b2;
            if (u1 != sp->expect_one || u2 != sp->expect_two) score = -987654321.0f;
        }
        const double r = score < 0 ? (double)score - 0.5 : (double)score + 0.5;
        o[pos] = (int)r;
    }
  }
}

// The same arrays, tiled: a workgroup takes 1 024 consecutive positions of one sequence and computes all four site types for
// them.  The four PSSMs, the residue -> column tables and the tile's residues (with the columns of every model looked up once)
// sit in LDS; a thread owns four consecutive positions and slides a four-byte window of columns along the model, so one LDS
// byte read serves four positions per model row; the four values of a position leave as 16-byte stores.  Every position's sum
// is the same chain of float adds in the same order as above (no reassociation), so the arrays are bit-identical; positions
// whose window is clipped by an end of the sequence take the one-by-one loop.  With `out16` (est2genome batches whose
// parameters allow the packed passes) the kernel also writes the packed passes' splice array -- the four values clamped to 16
// bits with the calc constant of a pre-splice transition folded in (fold[type]; ss16_kernel's formula) -- instead of a second
// pass that reads the 16 bytes per position back.
struct SpliceFold { int add[4]; };
constexpr int SPLICE_TILE = 1024, SPLICE_HALO = C4GPU_SPLICE_MAX_LEN;
__global__ __launch_bounds__(256) void splice_tile_kernel(const uint8_t *__restrict__ seq, const long long *off, const int *len, int n_seqs,
                                                          const c4gpu_splice_model *__restrict__ models, int *__restrict__ out,
                                                          long long stride, SpliceFold fold, uint2 *__restrict__ out16) {
    __shared__ float sdata[4][C4GPU_SPLICE_MAX_LEN * 5];
    __shared__ uint8_t sindex[4][256];
    __shared__ __attribute__((aligned(16))) uint8_t scol[4][SPLICE_TILE + 2 * SPLICE_HALO + 16];
    __shared__ __attribute__((aligned(16))) uint8_t sraw[SPLICE_TILE + 16];
    __shared__ int s_mlen[4], s_after[4], s_gtag[4], s_e1[4], s_e2[4];
    const int tid = threadIdx.x;
    for (int x = tid; x < 4 * C4GPU_SPLICE_MAX_LEN * 5; x += 256) sdata[x / (C4GPU_SPLICE_MAX_LEN * 5)][x % (C4GPU_SPLICE_MAX_LEN * 5)] =
        models[x / (C4GPU_SPLICE_MAX_LEN * 5)].data[(x % (C4GPU_SPLICE_MAX_LEN * 5)) / 5][x % 5];
    for (int x = tid; x < 4 * 256; x += 256) sindex[x >> 8][x & 255] = models[x >> 8].index[x & 255];
    if (tid < 4) {
        s_mlen[tid] = models[tid].model_length; s_after[tid] = models[tid].splice_after; s_gtag[tid] = models[tid].gtag_only;
        s_e1[tid] = models[tid].expect_one; s_e2[tid] = models[tid].expect_two;
    }
    __syncthreads();
    for (int pair = blockIdx.y; pair < n_seqs; pair += gridDim.y) {
        const uint8_t *s = seq + off[pair];
        const int n = len[pair];
        for (int tile = blockIdx.x * SPLICE_TILE; tile < n; tile += gridDim.x * SPLICE_TILE) {
            __syncthreads();                                   // the tile before has been read
            // residues tile - HALO .. tile + TILE + HALO as model columns (outside the sequence: never read), tile .. tile + TILE + 1 raw
            const int lo = tile - SPLICE_HALO;
            for (int x = tid; x < SPLICE_TILE + 2 * SPLICE_HALO; x += 256) {
                const int p = lo + x;
                const uint8_t b = (p >= 0 && p < n) ? s[p] : 0;
                for (int k = 0; k < 4; k++) scol[k][x] = sindex[k][b];
            }
            for (int x = tid; x < SPLICE_TILE + 2; x += 256) sraw[x] = (tile + x < n) ? s[tile + x] : 0;
            __syncthreads();
            const int p0 = tile + 4 * tid;                     // this thread's positions p0 .. p0 + 3
            if (p0 >= n) continue;
            int v[4][4];                                       // [type][position]
            for (int k = 0; k < 4; k++) {
                const int mlen = s_mlen[k], after = s_after[k];
                const float *d = sdata[k];
                const uint8_t *c = scol[k] + (p0 - after - lo);     // column of residue p0 - after + i at c[i]
                float sc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (p0 - after >= 0 && p0 + 3 - after + mlen <= n) {
                    unsigned w = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
                    for (int i = 0; i < mlen; i++) {
                        w |= (unsigned)c[i + 3] << 24;
                        const float *row = d + 5 * i;
                        sc[0] = sc[0] + row[w & 0xff];
                        sc[1] = sc[1] + row[(w >> 8) & 0xff];
                        sc[2] = sc[2] + row[(w >> 16) & 0xff];
                        sc[3] = sc[3] + row[w >> 24];
                        w >>= 8;
                    }
                } else {
                    for (int q = 0; q < 4; q++) {
                        const int pos = p0 + q;
                        if (pos >= n) break;
                        int seq_start = pos - after, model_start = 0, calc_length = mlen;
                        if (seq_start < 0) { model_start = -seq_start; seq_start = 0; calc_length -= model_start; }
                        if (seq_start + calc_length > n) calc_length = n - seq_start;
                        float score = 0.0f;
                        for (int i = 0; i < calc_length; i++) score = score + d[5 * (model_start + i) + scol[k][seq_start + i - lo]];
                        sc[q] = score;
                    }
                }
                for (int q = 0; q < 4; q++) {
                    float score = sc[q];
                    if (s_gtag[k]) {                            // Splice_predict_is_on_GTAG, splice.c:312-318 (past the end: the NUL)
                        const int pos = p0 + q;
                        const int b1 = sraw[4 * tid + q], b2 = pos + 1 < n ? sraw[4 * tid + q + 1] : 0;
                        const int u1 = (b1 >= 'a' && b1 <= 'z') ? b1 - 32 : b1, u2 = (b2 >= 'a' && b2 <= 'z') ? b2 - 32 : b2;
                        if (u1 != s_e1[k] || u2 != s_e2[k]) score = -987654321.0f;
                    }
                    const double r = score < 0 ? (double)score - 0.5 : (double)score + 0.5;
                    v[k][q] = (int)r;
                }
            }
            const long long base = off[pair] + p0;               // sequences start at multiples of four: 16-byte aligned
            if (p0 + 3 < n) {
                for (int k = 0; k < 4; k++)
                    *reinterpret_cast<int4 *>(out + (long long)k * stride + base) = make_int4(v[k][0], v[k][1], v[k][2], v[k][3]);
            } else {
                for (int k = 0; k < 4; k++)
                    for (int q = 0; q < 4 && p0 + q < n; q++) out[(long long)k * stride + base + q] = v[k][q];
            }
            if (out16) {
                auto c16 = [](int x) { return x < -32768 ? -32768 : (x > 32767 ? 32767 : x); };
                for (int q = 0; q < 4 && p0 + q < n; q++) {
                    uint2 o;
                    o.x = ((unsigned)c16(fold.add[0] + v[0][q]) & 0xffffu) | ((unsigned)c16(fold.add[1] + v[1][q]) << 16);
                    o.y = ((unsigned)c16(fold.add[2] + v[2][q]) & 0xffffu) | ((unsigned)c16(fold.add[3] + v[3][q]) << 16);
                    out16[base + q] = o;
                }
            }
        }
    }
}

// ---- resident sequences of a batch --------------------------------------------------------------------------
// Column entries of the blocked-cell lists (the device form of SubOpt_Index's rows, subopt.c:250-333): for
// every job and every column 0..T+1 two ints: the first blocked row of the column (or SUB_NONE), and twice
// the index of the first point at or after that column, plus 1 when the column holds more than one point.
__global__ void subopt_colptr_kernel(const DevJob *jobs, int n_jobs, const int *pts_t, const int *pts_q, int *colent) {
    // The points are sorted by column, so point k owns the columns after its predecessor's up to its own:
    // one pass of T+2 writes per job, no searches.
    constexpr int SUB_NONE = -0x40000000;
    for (int x = blockIdx.x; x < n_jobs; x += gridDim.x) {
        const DevJob &j = jobs[x];
        const int *pt = pts_t + j.sub_pt_off;
        const int *pq = pts_q + j.sub_pt_off;
        const int n = j.sub_pt_n;
        for (int k = threadIdx.x; k <= n; k += blockDim.x) {
            const int first = k == 0 ? 0 : pt[k - 1] + 1;
            const int last = k == n ? j.T + 1 : pt[k];          // inclusive
            const int idx2 = 2 * (j.sub_pt_off + k);
            for (int c = first; c <= last; c++) {
                const bool own = k < n && c == last;            // the column of point k itself
                const bool more = own && k + 1 < n && pt[k + 1] == c;
                int *e = colent + 2 * (j.sub_off + c);
                e[0] = own ? pq[k] : SUB_NONE;
                e[1] = idx2 | (more ? 1 : 0);
            }
        }
    }
}

// ---- sub-alignments of a checkpoint pass, listed and stitched on the device -------------------------------------
// Optimal_find_path_reduced_space (optimal.c:160-230) turns the checkpoint traceback of a region into a list of
// Viterbi_SubAlignments and Optimal_compute_subalignments (optimal.c:266-313) runs one FIND_PATH continuation per entry,
// each seeded with the final cell of the one before it.  A batch of 4 096 pairs of 1 kb x 1 kb under -D 32 has 778 443 of
// them: describing them on the host, uploading the descriptions and unpacking as many results was two thirds of a pass.
// The three kernels below keep that list on the device: the checkpoint kernel's DevVsa records become DevJobs
// (expand), the path kernel runs them, and one thread per pair checks every predicted final cell against the computed
// one and concatenates the runs in path order with Alignment_add's merge rule (stitch).  Pairs the fast route cannot
// finish (a section that itself needs checkpoints, a final cell that differs from its prediction, no END) are flagged
// and take the host route of find_path_batch.
enum { FUSE_MAX_OPS_CAP = 0, FUSE_MAX_TB, FUSE_MAX_T, FUSE_MAX_STRIPS, FUSE_OPS_TOTAL, FUSE_STATS };

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// one workgroup (one wave) per checkpoint job x; its children are out[first[x]] .. out[first[x + 1] - 1] in path order
__global__ __launch_bounds__(64) void fuse_expand_kernel(const DevJob *parents, const DevVsa *vsa, const int *first, int n_parents,
                                                         DevJob *out, c4h::MemRule rule, int dpmemory_mb, int path_R,
                                                         int *flags, unsigned long long *stats, int keep_root) {
    const int x = blockIdx.x;
    if (x >= n_parents) return;
    const DevJob &pj = parents[x];
    const int base = first[x], cnt = first[x + 1] - base;
    unsigned long long m_cap = 0, m_tb = 0, m_T = 0, m_strips = 0, ops = 0;
    bool nested = false;
    for (int k = threadIdx.x; k < cnt; k += 64) {
        const DevVsa &dv = vsa[pj.vsa_off + (cnt - 1 - k)];              // the list is last section first
        DevJob j;
        memset(&j, 0, sizeof j);
        j.pair = pj.pair; j.q0 = dv.qs; j.t0 = dv.ts; j.Q = dv.ql; j.T = dv.tl;
        j.root = keep_root ? pj.root : 0;    // the state the alignment's END is entered from (0: not known): BYROOT path kernels
        j.first_state = dv.first_state;
        // optimal.c:204-213,283-301: first cell = final cell of the sub-alignment before it (the parent's first cell for
        // the first one), final state = first state of the next one (the parent's final state for the last one)
        j.final_state = (k + 1 < cnt) ? vsa[pj.vsa_off + (cnt - 2 - k)].first_state : pj.final_state;
        const int *fc = k > 0 ? vsa[pj.vsa_off + (cnt - k)].final_cell : pj.first_cell;
        for (int l = 0; l < CELL_MAX; l++) j.first_cell[l] = fc[l];
        int tb = 0;
        while ((1LL << tb) <= j.T) tb++;
        j.tshift = tb;
        j.ckpt_off = -1; j.seed_off = -1;
        j.ops_cap = 3 * (j.Q + j.T) + 16;
        out[base + k] = j;
        nested |= c4h::use_reduced_space(rule, dv.ql, dv.tl, dpmemory_mb);
        const unsigned long long strips = (unsigned long long)(j.Q + 1 + 64 * path_R - 1) / (unsigned long long)(64 * path_R);
        const unsigned long long tbw = strips * (unsigned long long)(j.T + 64) * 64ull * (unsigned long long)path_R;
        m_cap = m_cap > (unsigned long long)j.ops_cap ? m_cap : (unsigned long long)j.ops_cap;
        m_tb = m_tb > tbw ? m_tb : tbw;
        m_T = m_T > (unsigned long long)j.T ? m_T : (unsigned long long)j.T;
        m_strips = m_strips > strips ? m_strips : strips;
        ops += (unsigned long long)j.ops_cap;
    }
    m_cap = wave_max_u64(m_cap); m_tb = wave_max_u64(m_tb); m_T = wave_max_u64(m_T); m_strips = wave_max_u64(m_strips);
    ops = wave_sum_u64(ops);
    const bool any_nested = __builtin_amdgcn_ballot_w64(nested) != 0;
    if (threadIdx.x == 0) {
        if (any_nested) flags[x] = 1;
        atomicMax(&stats[FUSE_MAX_OPS_CAP], m_cap); atomicMax(&stats[FUSE_MAX_TB], m_tb); atomicMax(&stats[FUSE_MAX_T], m_T);
        atomicMax(&stats[FUSE_MAX_STRIPS], m_strips); atomicAdd(&stats[FUSE_OPS_TOTAL], ops);
    }
}

// c4gpu_memrule_device: the rule on the device, one size per thread
__global__ void memrule_probe_kernel(c4h::MemRule rule, int dpmemory_mb, const int *ql, const int *tl, int n, int *reduced, int *rows) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    reduced[x] = c4h::use_reduced_space(rule, ql[x], tl[x], dpmemory_mb) ? 1 : 0;
    // the reference divides by the row size (viterbi.c:209): only defined where that size did not overflow
    rows[x] = c4h::viterbi_row_bytes(rule, ql[x], 1 + rule.total_shadow_designations + 1) ? c4h::checkpoint_rows(rule, ql[x], tl[x], dpmemory_mb) : -1;
}

// merged (transition, length) pairs at out[2 * off ..]; status bit 0: 0 = done; status >> 8: final cells of the pair that agreed
// with their predictions in everything but the score (final_cell_equiv's relaxation: counted for C4GPU_TRACE)
struct FusePair { long long off; int count, status; };

// Is the final cell a sub-alignment computed the one its successor was seeded with?  Exactly, except for cells predicted by the
// packed checkpoint pass (c4_ckpt16_kernel.h), whose intron-length counter saturates: a shadow slot (the target position an
// open intron started at) that lies 32 767 columns or more behind the cell is known there only as "that far back", and two
// such positions are interchangeable — the one thing ever computed from a shadow is the intron's length at its 3' site
// (intron.c:150-160), which passes the minimum either way and cannot exceed the maximum (Engine::pk16_fits).
//
// The SCORE of the cell is not compared (strict_score = false, the default; C4GPU_CELL_STRICT=1 compares it: the form of rounds
// 1-4).  A continuation sub-DP starts from ONE cell of ONE state (viterbi.c:705-714) and every score in it is that cell's
// score plus calcs along a path from it: max-plus is translation invariant, so a first cell whose score differs by d gives the
// same winners, the same ties, the same traceback and a final cell whose score differs by d and whose shadows are the same.
// The reference threads the computed cell through (optimal.c:283,301) and never looks at the checkpoint pass's score again;
// where intron length limits break optimal substructure the two differ by a few points (pair 3 775 of the all-against-all
// batch: 74 computed, 71 predicted, same intron start) -- the paths of every later sub-alignment are the ones the batch
// computed.  What does decide later cells are the shadow slots, and those are compared.  (Unset states hold -987654321
// whatever d is; a real candidate beats them by ~10^9 either way.)
__host__ __device__ inline bool final_cell_equiv(const int *computed, const int *predicted, int n_slots, int target_end, bool packed,
                                                 bool strict_score = false) {
    if (strict_score && computed[0] != predicted[0]) return false;
    // the argument is for plain max-plus; the one thing that is not translation invariant is a clamp (the -987654321 floor of
    // the protected calcs): a shift of a few points cannot reach it from any value a path cell holds (the kernels' guards keep
    // 4 x 10^8 between the two ranges), a large one is not what this relaxation is for and counts as a miss (ADVICE r05)
    const long long shift = (long long)computed[0] - (long long)predicted[0];
    if (shift > 4096 || shift < -4096) return false;
    for (int l = 1; l < n_slots; l++) {
        if (computed[l] == predicted[l]) continue;
        if (!(packed && (long long)target_end - predicted[l] - 2 >= 32767 && (long long)target_end - computed[l] - 2 >= 32767)) return false;
    }
    return true;
}

inline bool cell_strict() { return c4cfg::nonzero(c4cfg::CELL_STRICT); }

// one thread per checkpoint job: verify the chain of final cells, then Alignment_add (alignment.c:75-102) over the runs
// of its sub-alignments in path order (each job's walk wrote its runs END -> START)
__global__ void fuse_stitch_kernel(const DevJob *parents, const DevVsa *vsa, const int *first, int n_parents,
                                   const DevResult *sub, const uint32_t *runs, int path_cs, const int *flags,
                                   unsigned long long *out_used, int *out, FusePair *pairs, int n_packed, int strict_score) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_parents) return;
    FusePair fp; fp.off = 0; fp.count = 0; fp.status = 1;
    const int base = first[x], cnt = first[x + 1] - base;
    if (flags[x] || cnt == 0) { pairs[x] = fp; return; }
    const DevJob &pj = parents[x];
    long long total = 0;
    bool bad = false;
    int score_only = 0;
    for (int k = 0; k < cnt; k++) {
        const DevResult &r = sub[base + k];
        if (r.flags & (FLAG_OPS_OVERFLOW | FLAG_NO_END)) { bad = true; break; }
        total += r.n_ops;
        // the next sub-alignment was seeded with the predicted cell: it must be the one this one produced
        if (k + 1 < cnt) {
            const DevVsa &dv = vsa[pj.vsa_off + (cnt - 1 - k)];
            bad |= !final_cell_equiv(r.final_cell, dv.final_cell, path_cs, dv.ts + dv.tl, x < n_packed, strict_score != 0);
            if (bad) break;
            score_only += r.final_cell[0] != dv.final_cell[0];
        }
    }
    if (bad) { pairs[x] = fp; return; }
    const long long off = (long long)atomicAdd(out_used, (unsigned long long)total);
    int *o = out + 2 * off;
    int n = 0;
    for (int k = 0; k < cnt; k++) {
        const DevResult &r = sub[base + k];
        const uint32_t *w = runs + r.ops_off;
        for (int q = r.n_ops - 1; q >= 0; q--) {
            const int tr = (int)(w[q] >> 24), len = (int)(w[q] & 0xffffff);
            if (n && o[2 * (n - 1)] == tr) {
                o[2 * (n - 1) + 1] += len;
                if (o[2 * (n - 1) + 1] == 0) n--;
            } else {
                o[2 * n] = tr; o[2 * n + 1] = len; n++;
            }
        }
    }
    fp.off = off; fp.count = n; fp.status = score_only << 8;
    pairs[x] = fp;
}

// --annotation: the query positions [cds_start, cds_start + cds_length) of pair p (a DNA query with a CDS annotation,
// match.c:276-281) take row code 24 of the substitution matrix, the row that scores MATCH_IMPOSSIBLY_LOW_SCORE against
// everything (KParams::submat); one workgroup per pair
__global__ void annotate_qcode_kernel(uint8_t *qcode, const long long *qoff, const int *cds, int n_pairs) {
    const int p = blockIdx.x;
    if (p >= n_pairs) return;
    const int start = cds[3 * p], length = cds[3 * p + 1], qlen = cds[3 * p + 2];
    if (length <= 0) return;
    const int a = start < 0 ? 0 : start;
    const long long e = (long long)start + length;
    const int b = e > qlen ? qlen : (int)e;
    for (int i = a + (int)threadIdx.x; i < b; i += (int)blockDim.x) qcode[qoff[p] + i] = 24;
}

struct ResidentSeqs {
    int n_pairs = 0;
    std::vector<long long> qoff, toff;
    std::vector<int> qlen, tlen;
    long long total_q = 0, total_t = 0;
    DevBuf<uint8_t> qraw, traw, qcode, tcode;
    DevBuf<long long> d_qoff, d_toff;
    DevBuf<int> d_qlen, d_tlen, ss;
    DevBuf<uint16_t> tn4;
    mutable DevBuf<uint2> ss16;            // the packed score pass's splice values (built on its first launch over this batch)
    mutable bool ss16_built = false;
    mutable std::mutex ss16_lock;          // two lanes may reach the first packed launch together
    // the residue codes the targets hold, for the staged packed score pass (c4_viterbi16_kernel.h, IO 1): [0, 24) code -> dense
    // index (0xff: absent), [24, 32) dense index -> code; tdense_n = 0: not known (codon-coded targets)
    DevBuf<uint8_t> tdense;
    int tdense_n = 0;
    DevBuf<uint8_t> tcode_dense;          // the targets as dense indices into that table (dense_kernel); with tdense_n in 1 .. 8
    long long ss_len = 0;                 // positions per splice array
    DevBuf<PrepTables> tables;
    DevBuf<c4gpu_splice_model> splice_models;
    DevBuf<int> bad;
    DevSeqs dev;

    // Pairs that hand over the same host buffer (same pointer and length: one genomic contig against many
    // queries, all-vs-all front ends) share one device copy and one set of derived arrays.
    int n_utargets = 0;
    DevBuf<long long> d_utoff;
    DevBuf<int> d_utlen;
    // ... and the unique queries, for the families whose query is translated per sequence (family_is_codon)
    DevBuf<long long> d_uqoff;
    DevBuf<int> d_uqlen;

    // page-locked staging of the residues, kept between the batches of a c4gpu_stage (build with pin = true)
    PinBuf pin_q, pin_t;

    int build(c4gpu_ctx *ctx, int family, const c4gpu_params *params, const c4gpu_pair *pairs, int n, bool pin = false,
              const SpliceFold *fold16 = nullptr) {
        const bool trace = c4cfg::has(c4cfg::TRACE);
        const auto t_begin = std::chrono::steady_clock::now();
        auto lap = [&](const char *what) {
            if (trace) fprintf(stderr, "c4gpu trace: staging: %-24s at %.3f ms\n", what,
                               std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
        };
        n_pairs = n;
        qoff.resize(n); toff.resize(n); qlen.resize(n); tlen.resize(n);
        total_q = total_t = 0;
        std::map<std::pair<const uint8_t *, int>, long long> qseen, tseen;
        std::vector<int> uq, ut;                      // first pair that holds each unique sequence
        std::vector<long long> utoff, uqoff;          // (uqoff / uqlen: filled for the codon families only)
        std::vector<int> utlen, uqlen;
        for (int i = 0; i < n; i++) {
            qlen[i] = pairs[i].query_len; tlen[i] = pairs[i].target_len;
            if (qlen[i] < 0 || tlen[i] < 0 || tlen[i] >= (1 << 30) || qlen[i] >= (1 << 30)) {
                c4h::set_error("sequence length outside [0, 2^30): the kernels address a sequence with 32-bit byte offsets");
                return -1;
            }
            auto qk = std::make_pair(pairs[i].query, qlen[i]);
            auto qi = qseen.find(qk);
            if (qi == qseen.end()) {
                qseen[qk] = total_q; qoff[i] = total_q; uq.push_back(i);
                total_q += (qlen[i] + 3) & ~3LL;
            } else qoff[i] = qi->second;
            auto tk = std::make_pair(pairs[i].target, tlen[i]);
            auto ti = tseen.find(tk);
            if (ti == tseen.end()) {
                tseen[tk] = total_t; toff[i] = total_t; ut.push_back(i);
                utoff.push_back(total_t); utlen.push_back(tlen[i]);
                total_t += (tlen[i] + 3) & ~3LL;
            } else toff[i] = ti->second;
        }
        n_utargets = (int)ut.size();
        // one host buffer per side, every byte written exactly once (residues, 'A' in the gaps up to the next multiple
        // of four and in the 64-byte tail the kernels may read into) by several threads: a value-initialised vector of
        // this size (410 MB of targets for the north-star batch) is page-faulted in and written twice on one core.
        // A stage (c4gpu_stage: `pin` set) gathers into page-locked buffers it keeps between batches, slice by slice, each
        // slice on its way over the link while the next one is gathered.
        const size_t hq_n = (size_t)total_q + 64, ht_n = (size_t)total_t + 64;
        std::unique_ptr<uint8_t[]> own_q, own_t;
        uint8_t *hq = nullptr, *ht = nullptr;
        if (pin) {
            if (pin_q.reserve(hq_n) || pin_t.reserve(ht_n)) return -1;
            hq = pin_q.p; ht = pin_t.p;
        } else {
            own_q.reset(new uint8_t[hq_n]); own_t.reset(new uint8_t[ht_n]);
            hq = own_q.get(); ht = own_t.get();
        }
        hipStream_t s = ctx->stream;
        if (qraw.alloc(hq_n) || traw.alloc(ht_n)) return -1;
        // gathers the unique sequences [ua, ub) of one side; returns the byte range they cover
        auto gather = [&](uint8_t *dst, const std::vector<int> &uniq, bool query, size_t ua, size_t ub) {
            parallel_for((long long)(ub - ua), 16, [&](long long first, long long last) {
                for (long long x = (long long)ua + first; x < (long long)ua + last; x++) {
                    const int i = uniq[x];
                    const int len = query ? qlen[i] : tlen[i];
                    uint8_t *d = dst + (query ? qoff[i] : toff[i]);
                    if (len) memcpy(d, query ? pairs[i].query : pairs[i].target, len);
                    for (int k = len; k < ((len + 3) & ~3); k++) d[k] = 'A';
                }
            });
        };
        auto side = [&](uint8_t *host, uint8_t *devp, const std::vector<int> &uniq, bool query, long long total, size_t host_n) -> int {
            const size_t slice = pin ? (size_t)32 << 20 : ~(size_t)0;          // bytes per slice
            size_t ua = 0;
            long long sent = 0;
            while (ua < uniq.size()) {
                size_t ub = ua;
                long long end = sent;
                while (ub < uniq.size() && (size_t)(end - sent) < slice) {
                    const int i = uniq[ub++];
                    end = (query ? qoff[i] : toff[i]) + (((query ? qlen[i] : tlen[i]) + 3) & ~3LL);
                }
                gather(host, uniq, query, ua, ub);
                if (pin && end > sent) HIP_OK(hipMemcpyAsync(devp + sent, host + sent, (size_t)(end - sent), hipMemcpyHostToDevice, s));
                sent = end; ua = ub;
            }
            memset(host + total, 'A', 64);
            if (pin) HIP_OK(hipMemcpyAsync(devp + total, host + total, 64, hipMemcpyHostToDevice, s));
            else HIP_OK(hipMemcpyAsync(devp, host, host_n, hipMemcpyHostToDevice, s));
            return 0;
        };
        if (side(hq, qraw.p, uq, true, total_q, hq_n) || side(ht, traw.p, ut, false, total_t, ht_n)) return -1;
        lap("sequences gathered");
        PrepTables pt;
        memcpy(pt.submat_index, params->submat_index, 256);
        memcpy(pt.nt2d, params->nt2d, 256);
        memcpy(pt.trans, params->trans, 4096);
        memcpy(pt.aa, params->aa, 40);
        if (tables.upload(&pt, 1, s) ||
            qcode.alloc(hq_n) || tcode.alloc(ht_n) || d_qoff.upload(qoff.data(), n, s) ||
            d_toff.upload(toff.data(), n, s) || d_qlen.upload(qlen.data(), n, s) || d_tlen.upload(tlen.data(), n, s) ||
            d_utoff.upload(utoff.data(), n_utargets, s) || d_utlen.upload(utlen.data(), n_utargets, s))
            return -1;
        if (trace) { HIP_OK(c4_stream_sync(s)); lap("uploaded"); }
        int zero[2] = {0, 0};
        if (bad.upload(zero, 2, s)) return -1;
        const int blocks = 1024;
        int max_t = 1, max_q = 1;
        for (int i = 0; i < n; i++) { max_t = std::max(max_t, tlen[i]); max_q = std::max(max_q, qlen[i]); }
        if (family_is_codon(family)) {
            // Match_3_3 (match.c:508-530): the query is translated as the target of protein2dna is -- per position the row of
            // the residue its codon encodes (same table, same ambiguity handling; the last two positions start no codon).
            // Once per unique query, as the targets are.
            uqoff.resize(uq.size()); uqlen.resize(uq.size());
            for (size_t x = 0; x < uq.size(); x++) { uqoff[x] = qoff[uq[x]]; uqlen[x] = qlen[uq[x]]; }
            const int nuq = (int)uq.size();
            if (d_uqoff.upload(uqoff.data(), nuq, s) || d_uqlen.upload(uqlen.data(), nuq, s)) return -1;
            hipLaunchKernelGGL(codon_kernel, dim3(std::min(256, (max_q + 255) / 256), std::max(1, std::min(nuq, 32768))), dim3(256), 0, s,
                               qraw.p, qcode.p, d_uqoff.p, d_uqlen.p, nuq, tables.p, bad.p);
        } else {
            hipLaunchKernelGGL(encode_kernel, dim3(blocks), dim3(256), 0, s, qraw.p, qcode.p, (long long)hq_n, tables.p, bad.p);
        }
        const int xb = std::min(256, (max_t + 255) / 256), yb = std::max(1, std::min(n_utargets, 32768));
        if (family_is_p2d(family)) {
            hipLaunchKernelGGL(codon_kernel, dim3(xb, yb), dim3(256), 0, s, traw.p, tcode.p, d_utoff.p, d_utlen.p, n_utargets, tables.p, bad.p);
        } else {
            hipLaunchKernelGGL(encode_kernel, dim3(blocks), dim3(256), 0, s, traw.p, tcode.p, (long long)ht_n, tables.p, bad.p, bad.p + 1);
        }
        dev.ss = nullptr;
        dev.ss16 = nullptr;
        dev.ss_stride = 0;
        ss16_built = false;
        if (family_has_splice(family)) {
            if (splice_models.upload(params->splice, 4, s) || ss.alloc((size_t)4 * ht_n)) return -1;
            bool tiled = !(c4cfg::is(c4cfg::SPLICE_TILE, 0));     // 0: the one-position-per-thread kernel
            for (int k = 0; k < 4; k++)
                tiled = tiled && params->splice[k].splice_after >= 0 && params->splice[k].splice_after <= SPLICE_HALO &&
                        params->splice[k].model_length >= 0 && params->splice[k].model_length <= C4GPU_SPLICE_MAX_LEN;
            if (tiled) {
                if (fold16 && ss16.alloc(ht_n)) return -1;
                const int tiles = std::max(1, std::min(4096, (max_t + SPLICE_TILE - 1) / SPLICE_TILE));
                hipLaunchKernelGGL(splice_tile_kernel, dim3(tiles, yb), dim3(256), 0, s, traw.p, d_utoff.p, d_utlen.p, n_utargets,
                                   splice_models.p, ss.p, (long long)ht_n, fold16 ? *fold16 : SpliceFold{{0, 0, 0, 0}},
                                   fold16 ? ss16.p : (uint2 *)nullptr);
                if (fold16) { ss16_built = true; dev.ss16 = nullptr; }
            } else
            hipLaunchKernelGGL(splice_kernel, dim3(xb, yb, 4), dim3(256), 0, s, traw.p, d_utoff.p, d_utlen.p, n_utargets,
                               splice_models.p, ss.p, (long long)ht_n);
            dev.ss = ss.p;
            dev.ss_stride = (long long)ht_n;
            ss_len = (long long)ht_n;
        }
        dev.tn4 = nullptr;
        if (family_has_phase(family)) {
            if (tn4.alloc(ht_n)) return -1;
            hipLaunchKernelGGL(tn4_kernel, dim3(xb, yb), dim3(256), 0, s, traw.p, tn4.p, d_utoff.p, d_utlen.p, n_utargets, tables.p);
            dev.tn4 = tn4.p;
        }
        HIP_OK(hipGetLastError());
        lap("kernels queued");
        int hbad2[2] = {0, 0};
        if (bad.download(hbad2, 2, s)) return -1;
        HIP_OK(c4_stream_sync(s));
        const int hbad = hbad2[0];
        tdense_n = 0;
        if (!family_is_p2d(family) && hbad2[1]) {
            uint8_t tab[32];
            memset(tab, 0xff, 24);
            memset(tab + 24, 0, 8);
            int nd = 0;
            for (int c = 0; c < 24; c++)
                if (hbad2[1] >> c & 1) { if (nd < 8) { tab[c] = (uint8_t)nd; tab[24 + nd] = (uint8_t)c; } nd++; }
            if (nd <= 8) {
                if (tdense.upload(tab, 32, s) || tcode_dense.alloc(ht_n)) return -1;
                hipLaunchKernelGGL(dense_kernel, dim3(blocks), dim3(256), 0, s, tcode.p, tcode_dense.p, (long long)ht_n, tdense.p);
                HIP_OK(hipGetLastError());
                HIP_OK(c4_stream_sync(s));
                tdense_n = nd;
            }
        }
        lap("coded, splice arrays built");
        if (hbad) {
            c4h::set_error(hbad == 2 ? "a target codon translates outside the substitution matrix alphabet (non-IUPAC base?)"
                                     : "a residue is outside the 24-letter substitution matrix alphabet "
                                       "(exonerate's Submat index would read out of bounds, submat.c:27-61)");
            return -1;
        }
        dev.qcode = qcode.p; dev.tcode = tcode.p; dev.qoff = d_qoff.p; dev.toff = d_toff.p; dev.tlen = d_tlen.p;
        return 0;
    }

    // everything but the lock changes hands (c4gpu_batch_swap_stage: the batch takes the sequences a stage has loaded, the
    // stage takes the batch's old ones and loads the next batch into their buffers)
    void swap_with(ResidentSeqs &o) {
        std::swap(n_pairs, o.n_pairs);
        qoff.swap(o.qoff); toff.swap(o.toff); qlen.swap(o.qlen); tlen.swap(o.tlen);
        std::swap(total_q, o.total_q); std::swap(total_t, o.total_t);
        qraw.swap(o.qraw); traw.swap(o.traw); qcode.swap(o.qcode); tcode.swap(o.tcode);
        d_qoff.swap(o.d_qoff); d_toff.swap(o.d_toff); d_qlen.swap(o.d_qlen); d_tlen.swap(o.d_tlen); ss.swap(o.ss);
        tn4.swap(o.tn4); ss16.swap(o.ss16); std::swap(ss16_built, o.ss16_built);
        tdense.swap(o.tdense); std::swap(tdense_n, o.tdense_n); std::swap(ss_len, o.ss_len); tcode_dense.swap(o.tcode_dense);
        tables.swap(o.tables); splice_models.swap(o.splice_models); bad.swap(o.bad);
        std::swap(dev, o.dev);
        std::swap(n_utargets, o.n_utargets); d_utoff.swap(o.d_utoff); d_utlen.swap(o.d_utlen);
        d_uqoff.swap(o.d_uqoff); d_uqlen.swap(o.d_uqlen);
        std::swap(pin_q.p, o.pin_q.p); std::swap(pin_q.n, o.pin_q.n); std::swap(pin_t.p, o.pin_t.p); std::swap(pin_t.n, o.pin_t.n);
    }
};

