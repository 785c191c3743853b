/* c4gpu_seed.c — the word-scan seam of the drop-in (fifth file of the exonerate-gpu shim).
 *
 * The reference's Seeder_add_target (src/comparison/seeder.c:852-915) walks every target — for translated matches its
 * three translated frames — through the automaton the queries built (FSM_traverse src/struct/fsm.c:186-198, or
 * Seeder_VFSM_traverse_single seeder.c:698-720) on one host core and calls Seeder_FSM_traverse_func (seeder.c:649-695) at
 * every word end, which hands each seed of the word and of its neighbours to HSPset_seed_hsp.  This front of
 * Seeder_add_target (seeder.o keeps its own under Seeder_add_target_cpu) does the same with the walk on the device:
 *   1. ONCE per seeder, before the automaton is compiled: the words the queries put into it, read off the trie
 *      (FSM, pre-compile: fsm.c:112-135) or the leaf table (VFSM), each with its emission list in the reference's order —
 *      the word's own seeds, then the seeds of each neighbour (seeder.c:676-692) — go into a c4gpu_wordtab; the automaton
 *      is then compiled as Seeder_prepare would (seeder.c:779-784), so the reference's own walk stays usable;
 *   2. per target / frame: the string the reference would walk (Sequence_mask, Sequence_translate: its own functions),
 *      mapped through the automaton's traversal filter to column numbers, goes to c4gpu_seed_scan; the hits come back in
 *      walk order and are handed to HSPset_seed_hsp exactly as Seeder_WordInfo_seed does (seeder.c:624-647) — whose
 *      front (c4gpu_hsp.c) batches the extensions on the device;
 *   3. the report loop of Seeder_add_target (seeder.c:899-913) follows unchanged.
 * Building the automaton (Seeder_add_query, word neighbourhoods) stays the reference's; with C4GPU_SEED_BUILD=1 (opt-in, below)
 * step 1 does not read it but builds the table on the device from the queries (c4gpu_wordtab_build).  Not taken (the reference's own
 * function runs): --saturatethreshold (a per-word running count in walk order), --wordambiguity > 1, seeders with both
 * a DNA and a codon loader, a seeder whose automaton was compiled before this front saw it, and -- unless C4GPU_CODON_SEED=1
 * (opt-in) -- a seeder with a translated query (ungapped:trans, coding2coding: the words of the query's three frames in one
 * automaton, their seeds' query positions nucleotide positions already, seeder.c:540-545; the table reads them as they are).
 * C4GPU_SEED_FUSED=1 (opt-in): where every emission of the table belongs to one loader whose HSP_Param
 * uses a horizon (DNA / protein / protein-vs-DNA -- with C4GPU_CODON_SEED=1 also codon-vs-codon without an annotated query --,
 * with C4GPU_SEED_FUSED_OPT=1 beside it also soft-masked alphabets, and --seedrepeat > 1 where query and target advance are equal,
 * so not protein-vs-DNA) step 2 is ONE
 * c4gpu_seed_extend_opt call per target -- scan, horizon test, extension and threshold on the device, the hits never leaving it --
 * and only the HSPs a fresh HSPset per query would store come back, in walk order; each goes to HSPset_add_known_hsp of its
 * query's set; the Comparisons are created in the order of the queries' first word hits (c4gpu_seed_extend_first_hits), which is
 * the order Seeder_WordInfo_seed creates them in and the report loop follows.  A query whose hits all fall away gets no
 * Comparison (the reference makes one and destroys it unreported).  With C4GPU_SEED_HOST=1 the kept list comes from the
 * reference's own HSPset_seed_hsp on one scratch set per query, fed the host scan's seeds in order.  A call that fails leaves
 * nothing delivered: the target takes the scan and extension calls below.  Not with C4GPU_SEED_CHECK / C4GPU_HSP_CHECK.
 * C4GPU_SEED_OFF=1 switches the seam off; C4GPU_SEED_HOST=1 replaces the device scan by a dictionary scan on the host
 * (CPU test of steps 1 and 3); C4GPU_SEED_CHECK=1 also runs the reference's own walk first and compares the two hit lists
 * seed for seed (abort on the first difference).
 */
#include <string.h>
#include <stdlib.h>
#include <ctype.h>

#include "seeder.h"
#include "comparison.h"
#include "hspset.h"
#include "sequence.h"
#include "fsm.h"
#include "vfsm.h"
#include "submat.h"
#include "alphabet.h"
#include "wordhood.h"

#include "c4gpu.h"
#include "c4gpu_shim.h"

extern void Seeder_add_target_cpu(Seeder *seeder, Sequence *target);
extern void HSPset_seed_hsp_cpu(HSPset *hsp_set, guint query_start, guint target_start);
extern void Seeder_destroy_cpu(Seeder *seeder);

typedef struct { Seeder_QueryInfo *query_info; Seeder_Loader *loader; gint query_pos; } ShimEmit;
typedef struct { Sequence *query; HSP_Param *param; guint query_pos, target_pos; } ShimSeedRec;

typedef struct {
    Seeder *seeder;
    gboolean usable, hopeless;           /* table built / this seeder keeps the reference's walk */
    gint64 walked;                        /* symbols the reference's walk has seen while the table was not worth building */
    gint width, wordlen;
    guchar column[ALPHABETSIZE];          /* residue -> automaton column (0: outside the alphabet) */
    gboolean upper;                       /* the VFSM walk upper-cases (seeder.c:704) */
    GArray *codes, *first, *emits;        /* guint64 per word; gint32 n_words + 1; ShimEmit */
    GHashTable *host_index;               /* C4GPU_SEED_HOST: code -> word number + 1 */
    c4gpu_wordtab *tab;
    /* C4GPU_SEED_FUSED: the one loader all emissions belong to (NULL: several, or its HSP_Param is not served), the emissions
     * as (index in the seeder's query list, query position), the queries' residues, whether the device table has them */
    gboolean fused_looked;
    Seeder_Loader *fused_loader;
    c4gpu_seed_emit *fused_emits;
    gchar **fused_query;
    gboolean fused_sent;
} ShimSeedTab;

static GHashTable *seed_tabs = NULL;      /* Seeder* -> ShimSeedTab* */
static GArray *seed_record = NULL;        /* C4GPU_SEED_CHECK: what the reference's own walk hands to HSPset_seed_hsp */
static struct { long targets, cpu_targets, scans, symbols, hits, checked, words, emits; double scan_ms, host_ms, table_ms;
                long fused_targets, fused_hits, fused_extended, fused_kept; double fused_ms;
                long read, built; double build_ms; } sdst;

gboolean shim_seed_recording(HSPset *hsp_set, guint query_start, guint target_start){
    ShimSeedRec r;
    if(!seed_record)
        return FALSE;
    r.query = hsp_set->query; r.param = hsp_set->param; r.query_pos = query_start; r.target_pos = target_start;
    g_array_append_val(seed_record, r);
    return TRUE;
    }

static void seed_emit_word(ShimSeedTab *st, Seeder_WordInfo *word_info){
    register Seeder_Seed *seed;
    register Seeder_Neighbour *neighbour;
    ShimEmit e;
    for(seed = word_info->seed_list; seed; seed = seed->next){
        e.query_info = seed->context->query_info; e.loader = seed->context->loader; e.query_pos = seed->query_pos;
        g_array_append_val(st->emits, e);
        }
    for(neighbour = word_info->neighbour_list; neighbour; neighbour = neighbour->next)
        for(seed = neighbour->word_info->seed_list; seed; seed = seed->next){
            e.query_info = seed->context->query_info; e.loader = seed->context->loader; e.query_pos = seed->query_pos;
            g_array_append_val(st->emits, e);
            }
    return;
    }

static void seed_add_word(ShimSeedTab *st, guint64 code, Seeder_WordInfo *word_info){
    gint32 n;
    g_array_append_val(st->codes, code);
    seed_emit_word(st, word_info);
    n = st->emits->len;
    g_array_append_val(st->first, n);
    return;
    }

/* The last level of the walk: every word's code and the seeds it emits (its own, then those of its neighbours: seed_emit_word).
 * Three dependent loads into cold memory per word -- 0.23 us each, 130 ms for the 570 000 words of a 128-protein seeder on one
 * thread.  The nodes are read-only here and the words of different nodes are independent: slices of the node list go to a few
 * threads, each with a table of its own, and the tables are joined in slice order (so the numbering is that of the one-thread
 * walk).  C4GPU_SEED_THREADS=1: one thread. */
typedef struct { FSM_Node *node; guint64 code; } ShimTrieItem;
typedef struct { ShimSeedTab part; FSM *f; ShimTrieItem *item; guint n; } ShimWordSlice;
static void seed_read_slice(ShimSeedTab *st, FSM *f, ShimTrieItem *item, guint n){
    register guint k;
    register gint c;
    for(k = 0; k < n; k++)
        for(c = 1; c < f->width; c++)
            if(item[k].node[c].data)
                seed_add_word(st, item[k].code * f->width + c, item[k].node[c].data);
    return;
    }
static gpointer seed_read_slice_thread(gpointer data){
    register ShimWordSlice *sl = data;
    seed_read_slice(&sl->part, sl->f, sl->item, sl->n);
    return NULL;
    }
static void seed_read_words(ShimSeedTab *st, FSM *f, GArray *words){
    register gint n_threads = shim_num(C4GPU_SEED_THREADS, (gint)MIN(8, g_get_num_processors()));
    register gint t;
    register guint k;
    ShimWordSlice *sl;
    GThread **th;
    if((n_threads < 2) || (words->len < (shim_has(C4GPU_SEED_THREADS) ? (guint)n_threads : 4096u))){     /* (asked for: any size) */
        seed_read_slice(st, f, (ShimTrieItem*)words->data, words->len);
        return;
        }
    sl = g_new0(ShimWordSlice, n_threads);
    th = g_new0(GThread*, n_threads);
    for(t = 0; t < n_threads; t++){
        register guint lo = (guint)(((guint64)words->len * t) / n_threads), hi = (guint)(((guint64)words->len * (t + 1)) / n_threads);
        gint32 zero = 0;
        sl[t].f = f;
        sl[t].item = ((ShimTrieItem*)words->data) + lo;
        sl[t].n = hi - lo;
        sl[t].part.codes = g_array_new(FALSE, FALSE, sizeof(guint64));
        sl[t].part.first = g_array_new(FALSE, FALSE, sizeof(gint32));
        sl[t].part.emits = g_array_new(FALSE, FALSE, sizeof(ShimEmit));
        g_array_append_val(sl[t].part.first, zero);
        th[t] = g_thread_new("c4gpu-words", seed_read_slice_thread, &sl[t]);
        }
    for(t = 0; t < n_threads; t++){
        register gint32 base = st->emits->len;
        g_thread_join(th[t]);
        g_array_append_vals(st->codes, sl[t].part.codes->data, sl[t].part.codes->len);
        g_array_append_vals(st->emits, sl[t].part.emits->data, sl[t].part.emits->len);
        for(k = 1; k < sl[t].part.first->len; k++){          /* (entry 0 is the slice's own leading zero) */
            gint32 v = base + g_array_index(sl[t].part.first, gint32, k);
            g_array_append_val(st->first, v);
            }
        g_array_free(sl[t].part.codes, TRUE);
        g_array_free(sl[t].part.first, TRUE);
        g_array_free(sl[t].part.emits, TRUE);
        }
    g_free(sl);
    g_free(th);
    return;
    }

/* The words of the automaton, level by level.  Before FSM_compile (fsm.c:136-184) `next` is NULL where the trie has no
 * child; after it every `next` is set, but a failure link leads to a node no deeper than its origin, so in a level-order
 * walk the edges into nodes not seen before are exactly the trie's own: the walk reads both forms.  Column c of a node at
 * the last level holds the word's data. */
static void seed_walk_trie(ShimSeedTab *st, FSM *f){
    register GArray *level = g_array_new(FALSE, FALSE, sizeof(ShimTrieItem)), *next_level, *words;
    /* (before FSM_compile every non-NULL `next` is a trie edge: no need to remember the nodes seen -- a hash insertion per node
     * was half of the 130 ms a 256-protein seeder's 1.7 million words took to read) */
    register GHashTable *seen = f->is_compiled ? g_hash_table_new(g_direct_hash, g_direct_equal) : NULL;
    register gint depth, c;
    register guint k;
    ShimTrieItem it;
    it.node = f->root; it.code = 0;
    g_array_append_val(level, it);
    if(seen)
        g_hash_table_insert(seen, f->root, f->root);
    for(depth = 0; depth + 1 < st->wordlen; depth++){
        next_level = g_array_new(FALSE, FALSE, sizeof(ShimTrieItem));
        for(k = 0; k < level->len; k++){
            register ShimTrieItem *p = &g_array_index(level, ShimTrieItem, k);
            for(c = 1; c < f->width; c++){
                register FSM_Node *child = p->node[c].next;
                if(child && ((!seen) || !g_hash_table_lookup(seen, child))){
                    if(seen)
                        g_hash_table_insert(seen, child, child);
                    it.node = child; it.code = p->code * f->width + c;
                    g_array_append_val(next_level, it);
                    }
                }
            }
        g_array_free(level, TRUE);
        level = next_level;
        }
    if(seen)
        g_hash_table_destroy(seen);
    /* the reference's traversal meets the words in no particular order; ours does not depend on it either (hash table) */
    words = level;
    seed_read_words(st, f, words);
    g_array_free(words, TRUE);
    return;
    }

/* Is the table worth building yet?  Reading the words off the automaton costs about as much as the reference's walk over
 * a few symbols per trie node; until the targets of this seeder add up to that, the reference's own walk serves them (a
 * 100-protein seeder with word neighbourhoods against one 10 kaa target is walked in a millisecond and its 660 000 words
 * would take 270 ms to read).  The factor was 16 until round 4 (0.5 us per node against 20-50 ns per walked symbol, measured
 * on short targets); config 5's heuristic leg measured it again on a 10 Mb chromosome (profiles/r04_c5_breakdown.md): the
 * reference's three-frame walk of 10 Mb is 700-800 ms, reading a 256-protein seeder's words 200 ms and scanning the
 * chromosome on the device 100 ms with delivery -- break-even at 2.7 symbols per node, and with 16 the first strand of every
 * query chunk was still walked on the CPU.  Now 4 (C4GPU_SEED_FACTOR). */
static gboolean seed_worth_it(ShimSeedTab *st, Sequence *target){
    register Seeder *seeder = st->seeder;
    register gdouble nodes = seeder->seeder_fsm ? (gdouble)seeder->seeder_fsm->fsm->chunk_count
                                                : (gdouble)seeder->seeder_vfsm->vfsm->lrw / 64.0;
    register gdouble factor = shim_real(C4GPU_SEED_FACTOR, 4.0);
    return (gdouble)(st->walked + target->len) >= factor * nodes;
    }

static ShimSeedTab *seed_state(Seeder *seeder){
    register ShimSeedTab *st;
    if(!seed_tabs)
        seed_tabs = g_hash_table_new(g_direct_hash, g_direct_equal);
    if((st = g_hash_table_lookup(seed_tabs, seeder)))
        return st;
    st = g_new0(ShimSeedTab, 1);
    st->seeder = seeder;
    g_hash_table_insert(seed_tabs, seeder, st);
    if(seeder->saturate_threshold || (seeder->sas->word_ambiguity > 1) || (seeder->dna_loader && seeder->codon_loader))
        st->hopeless = TRUE;
    return st;
    }

/* ---- C4GPU_SEED_BUILD=1 (opt-in): step 1 on the device ----
 * The word table comes from c4gpu_wordtab_build, fed the seeder's own queries, instead of being read off the automaton word by
 * word.  For a seeder with exactly one loader, no codon loader, no saturate threshold, a word jump of 1 and no annotated query
 * (Seeder_word_is_valid); any other seeder takes the trie read as before.  The reference's Seeder_add_query has still run -- its
 * memory accounting (seeder.c:612) decides where a query chunk ends, and its walk stays the fallback -- so this switch does NOT
 * remove the host automaton: it removes reading it.  C4GPU_SEED_BUILD_CHECK=1 also reads the trie and compares the two tables
 * word for word and emission for emission. */
static gboolean seed_build_wanted(ShimSeedTab *st){
    register Seeder *seeder = st->seeder;
    register guint k;
    if((!shim_nonzero(C4GPU_SEED_BUILD)) || shim_has(C4GPU_SEED_HOST))
        return FALSE;
    if(seeder->codon_loader || seeder->saturate_threshold || (seeder->sas->word_jump != 1)
    || ((seeder->dna_loader ? 1 : 0) + (seeder->protein_loader ? 1 : 0) != 1))
        return FALSE;
    for(k = 0; k < seeder->query_info_list->len; k++)
        if(((Seeder_QueryInfo*)seeder->query_info_list->pdata[k])->query->annotation)
            return FALSE;
    return TRUE;
    }

/* st->width / st->column are set.  Fills st->codes / first / emits from the exported table and leaves the table in st->tab */
static gboolean seed_build_device(ShimSeedTab *st){
    register Seeder *seeder = st->seeder;
    register Seeder_Loader *loader = seeder->dna_loader ? seeder->dna_loader : seeder->protein_loader;
    register HSP_Param *param = loader->hsp_param;
    register Match *match = param->match;
    register gboolean translated = match->query->is_translated;
    register gint n_queries = seeder->query_info_list->len, n_strings = n_queries * (translated ? 3 : 1), i, a, b;
    register guchar **sym = g_new0(guchar*, n_strings + 1);
    register gint32 *n_sym = g_new0(gint32, n_strings + 1);
    register c4gpu_word_source *src = g_new0(c4gpu_word_source, n_strings + 1);
    register gint32 *scores = NULL;
    register gboolean ok = TRUE;
    register guint64 *codes;
    register c4gpu_seed_emit *emits;
    register gint32 *first;
    c4gpu_wordtab_build_stats stats;
    int64_t n_words = 0, n_emits = 0;
    guchar insert[ALPHABETSIZE];
    /* the column a query symbol is inserted under, 0 exactly where seeder.c:501-514 resets */
    for(i = 0; i < ALPHABETSIZE; i++){
        if(seeder->seeder_fsm){
            insert[i] = Alphabet_symbol_is_member(match->comparison_alphabet, i) ? seeder->seeder_fsm->fsm->insertion_filter[i] : 0;
        } else
            insert[i] = st->column[i];
        }
    insert[0] = 0;
    for(i = 0; ok && (i < n_strings); i++){
        register Seeder_QueryInfo *query_info = seeder->query_info_list->pdata[translated ? i / 3 : i];
        register Sequence *seq = translated ? Sequence_translate(query_info->query, match->mas->translate, (i % 3) + 1)
                                            : Sequence_share(query_info->query);
        register Sequence *masked = Sequence_mask(seq);           /* seeder.c:486-487 */
        register gchar *str = Sequence_get_str(masked);
        register gint x;
        n_sym[i] = seq->len;
        sym[i] = g_new(guchar, n_sym[i] + 1);
        for(x = 0; x < n_sym[i]; x++){
            sym[i][x] = insert[(guchar)str[x]];
            /* (a member the trie has no column for: FSM_add ends the run on such a word, fsm.c:109-111; not met after Seeder_add_query) */
            if(seeder->seeder_fsm && (!sym[i][x]) && Alphabet_symbol_is_member(match->comparison_alphabet, (guchar)str[x]))
                ok = FALSE;
            }
        src[i].pair = translated ? i / 3 : i;
        src[i].pos_scale = translated ? 3 : 1;                    /* seeder.c:540-543 */
        src[i].pos_offset = translated ? i % 3 : 0;
        g_free(str);
        Sequence_destroy(masked);
        Sequence_destroy(seq);
        }
    if(ok && param->wordhood){                                    /* hspset.c:146-167: the loader's submat over the alphabet's members */
        register Submat *submat = (match->type == Match_Type_DNA2DNA) ? match->mas->dna_submat : match->mas->protein_submat;
        register const guchar *member = match->comparison_alphabet->member;
        guchar letter[ALPHABETSIZE];
        memset(letter, 0, sizeof(letter));
        for(i = 0; member[i]; i++)
            letter[insert[member[i]]] = member[i];
        scores = g_new0(gint32, st->width * st->width);
        for(a = 1; a < st->width; a++)
            for(b = 1; b < st->width; b++)
                if(letter[a] && letter[b])
                    scores[a * st->width + b] = Submat_lookup(submat, letter[a], letter[b]);
        }
    if(ok){
        st->tab = c4gpu_wordtab_build(shim_get_ctx(), st->width, st->wordlen, (const uint8_t *const *)sym, n_sym, src, n_strings, scores,
                                      param->wordhood ? param->wordhood->threshold : 0,
                                      param->wordhood ? (param->wordhood->use_dropoff ? 1 : 0) : 1, &stats);
        if(!st->tab){
            g_warning("c4gpu: %s -- the word table is read off the automaton", c4gpu_last_error());
            ok = FALSE;
            }
        }
    for(i = 0; i < n_strings; i++)
        g_free(sym[i]);
    g_free(sym); g_free(n_sym); g_free(src); g_free(scores);
    if(!ok)
        return FALSE;
    codes = g_new(guint64, stats.n_words + 1);
    first = g_new(gint32, stats.n_words + 2);
    emits = g_new(c4gpu_seed_emit, stats.n_emits + 1);
    if((c4gpu_wordtab_export(shim_get_ctx(), st->tab, (uint64_t*)codes, first, stats.n_words, emits, stats.n_emits, &n_words, &n_emits) != 0)
    || (n_words != stats.n_words) || (n_emits != stats.n_emits)){
        g_warning("c4gpu: %s -- the word table is read off the automaton", c4gpu_last_error());
        c4gpu_wordtab_destroy(st->tab);
        st->tab = NULL;
        ok = FALSE;
        }
    if(ok){
        g_array_set_size(st->codes, 0); g_array_set_size(st->first, 0); g_array_set_size(st->emits, 0);
        g_array_append_vals(st->codes, codes, n_words);
        g_array_append_vals(st->first, first, n_words + 1);
        for(i = 0; i < n_emits; i++){
            ShimEmit e;
            e.query_info = seeder->query_info_list->pdata[emits[i].pair]; e.loader = loader; e.query_pos = emits[i].query_pos;
            g_array_append_val(st->emits, e);
            }
        st->fused_sent = TRUE;                                     /* the built table has its emissions: nothing to send again */
        sdst.built++; sdst.build_ms += stats.build_ms;
        }
    g_free(codes); g_free(first); g_free(emits);
    return ok;
    }

/* C4GPU_SEED_BUILD_CHECK: `st` holds the table read off the automaton, `b_*` the built one */
static void seed_build_check(ShimSeedTab *st, GArray *b_codes, GArray *b_first, GArray *b_emits){
    register guint k, w = 0, n = 0;
    register glong mismatches = 0;
    for(k = 0; k < st->codes->len; k++){
        register gint32 lo = g_array_index(st->first, gint32, k), hi = g_array_index(st->first, gint32, k + 1), e;
        if(hi == lo)
            continue;                                              /* a word without emissions is not a word of the table */
        n++;
        if((w >= b_codes->len) || (g_array_index(b_codes, guint64, w) != g_array_index(st->codes, guint64, k))
        || ((g_array_index(b_first, gint32, w + 1) - g_array_index(b_first, gint32, w)) != (hi - lo))){
            mismatches++;
            if((w < b_codes->len) && (g_array_index(b_codes, guint64, w) <= g_array_index(st->codes, guint64, k)))
                w++;
            continue;
            }
        for(e = 0; e < hi - lo; e++){
            register ShimEmit *x = &g_array_index(st->emits, ShimEmit, lo + e);
            register ShimEmit *y = &g_array_index(b_emits, ShimEmit, g_array_index(b_first, gint32, w) + e);
            if((x->query_info != y->query_info) || (x->loader != y->loader) || (x->query_pos != y->query_pos))
                mismatches++;
            }
        w++;
        }
    mismatches += b_codes->len - w;
    g_message("c4gpu seed: build check %u words, %ld mismatches", n, mismatches);
    return;
    }

static gboolean seed_build(ShimSeedTab *st){
    register Seeder *seeder = st->seeder;
    register gint i;
    gint32 zero = 0;
    gint64 t_begin = g_get_monotonic_time();
    GArray *b_codes = NULL, *b_first = NULL, *b_emits = NULL;
    st->wordlen = seeder->any_hsp_param->wordlen;
    st->codes = g_array_new(FALSE, FALSE, sizeof(guint64));
    st->first = g_array_new(FALSE, FALSE, sizeof(gint32));
    st->emits = g_array_new(FALSE, FALSE, sizeof(ShimEmit));
    if(seed_build_wanted(st) && ((!seeder->seeder_vfsm) || ((gint)seeder->seeder_vfsm->vfsm->depth == st->wordlen))){
        if(seeder->seeder_fsm){
            st->width = seeder->seeder_fsm->fsm->width;
            for(i = 0; i < ALPHABETSIZE; i++)
                st->column[i] = seeder->seeder_fsm->fsm->traversal_filter[i];
        } else {
            st->width = seeder->seeder_vfsm->vfsm->alphabet_size + 1;
            st->upper = TRUE;
            for(i = 0; i < ALPHABETSIZE; i++)
                st->column[i] = (guchar)seeder->seeder_vfsm->vfsm->index[toupper(i)];
            }
        st->column[0] = 0;
        if(seed_build_device(st)){
            shim_mark("  word table built on the device");
            if(!seeder->seeder_fsm)
                seeder->is_prepared = TRUE;
            if(!shim_has(C4GPU_SEED_BUILD_CHECK)){
                st->usable = TRUE;
                sdst.words += st->codes->len; sdst.emits += st->emits->len;
                sdst.table_ms += (g_get_monotonic_time() - t_begin) / 1e3;
                return TRUE;
                }
            /* the check: what follows reads the automaton as ever, into arrays of its own */
            b_codes = st->codes; b_first = st->first; b_emits = st->emits;
            st->codes = g_array_new(FALSE, FALSE, sizeof(guint64));
            st->first = g_array_new(FALSE, FALSE, sizeof(gint32));
            st->emits = g_array_new(FALSE, FALSE, sizeof(ShimEmit));
            }
        }
    g_array_set_size(st->codes, 0); g_array_set_size(st->first, 0); g_array_set_size(st->emits, 0);
    g_array_append_val(st->first, zero);
    sdst.read++;
    if(seeder->seeder_fsm){
        register FSM *f = seeder->seeder_fsm->fsm;
        st->width = f->width;
        for(i = 0; i < ALPHABETSIZE; i++)
            st->column[i] = f->traversal_filter[i];
        st->column[0] = 0;
        seed_walk_trie(st, f);
        shim_mark("  trie read");
        /* FSM_compile (Seeder_prepare, seeder.c:783-788) is left to the reference's own walk, which prepares the seeder when it is
         * first asked (seeder.c:865) -- that is only where a scan could not be served.  The failure links are of no use to the
         * word table, and compiling a 256-protein seeder's automaton took as long as reading its words (C4GPU_SEED_COMPILE=1:
         * compile here, as rounds 3-4 did) */
        if((!f->is_compiled) && shim_has(C4GPU_SEED_COMPILE)){
            FSM_compile(f);
            seeder->is_prepared = TRUE;
            shim_mark("  automaton compiled");
            }
    } else {
        register VFSM *vfsm = seeder->seeder_vfsm->vfsm;
        register VFSM_Int leaf;
        register gchar *word = g_new0(gchar, vfsm->depth + 1);
        st->width = vfsm->alphabet_size + 1;
        st->upper = TRUE;
        for(i = 0; i < ALPHABETSIZE; i++)
            st->column[i] = (guchar)vfsm->index[toupper(i)];
        st->column[0] = 0;
        if((gint)vfsm->depth != st->wordlen){
            g_free(word);
            return FALSE;
            }
        for(leaf = 0; leaf < vfsm->lrw; leaf++){
            register Seeder_WordInfo *word_info = seeder->seeder_vfsm->leaf[leaf];
            register guint64 code = 0;
            if(!word_info)
                continue;
            VFSM_state2word(vfsm, VFSM_leaf2state(vfsm, leaf), word);
            for(i = 0; i < st->wordlen; i++)
                code = code * st->width + (guchar)vfsm->index[(guchar)word[i]];
            seed_add_word(st, code, word_info);
            }
        g_free(word);
        }
    if(!seeder->seeder_fsm)
        seeder->is_prepared = TRUE;                            /* (nothing to compile: Seeder_prepare only sets the flag) */
    if(b_codes){                                               /* C4GPU_SEED_BUILD_CHECK: compare, then go on with the built table */
        seed_build_check(st, b_codes, b_first, b_emits);
        g_array_free(st->codes, TRUE); g_array_free(st->first, TRUE); g_array_free(st->emits, TRUE);
        st->codes = b_codes; st->first = b_first; st->emits = b_emits;
    } else if(shim_has(C4GPU_SEED_HOST)){
        st->host_index = g_hash_table_new(g_int64_hash, g_int64_equal);
        for(i = 0; i < (gint)st->codes->len; i++)
            g_hash_table_insert(st->host_index, &g_array_index(st->codes, guint64, i), GINT_TO_POINTER(i + 1));
    } else {
        st->tab = c4gpu_wordtab_create(shim_get_ctx(), st->width, st->wordlen, (const uint64_t*)st->codes->data,
                                       (const int32_t*)st->first->data, st->codes->len);
        shim_mark("  word table on the device");
        if(!st->tab){
            g_warning("c4gpu: %s -- the word scan stays on the CPU", c4gpu_last_error());
            return FALSE;
            }
        }
    st->usable = TRUE;
    sdst.words += st->codes->len; sdst.emits += st->emits->len;
    sdst.table_ms += (g_get_monotonic_time() - t_begin) / 1e3;
    return TRUE;
    }

/* Seeder_WordInfo_seed, seeder.c:624-647 (no saturation threshold here) */
static void seed_deliver(Seeder *seeder, Sequence *target, ShimEmit *e, gint target_pos, GArray *mine){
    register Seeder_QueryInfo *query_info = e->query_info;
    register HSPset *hspset;
    seeder->comparison_count++;
    if(!query_info->curr_comparison){
        query_info->curr_comparison = Comparison_create(seeder->comparison_param, query_info->query, target);
        g_ptr_array_add(seeder->active_queryinfo_list, query_info);
        }
    hspset = *(HSPset**)((gchar*)query_info->curr_comparison + e->loader->hspset_offset);   /* OFFSET_ITEM, seeder.c:644 */
    if(mine){
        ShimSeedRec r;
        r.query = hspset->query; r.param = hspset->param; r.query_pos = e->query_pos; r.target_pos = target_pos;
        g_array_append_val(mine, r);
        }
    HSPset_seed_hsp(hspset, e->query_pos, target_pos);
    return;
    }

/* one walk: `seq` as the reference would hand it to FSM_traverse, frame 0 (untranslated) or 1 .. 3.  The hits of a frame are
 * only written down here; Seeder_add_target delivers them once every frame of the target has been scanned, so that a scan
 * that fails (no device memory for the hit buffer, a HIP error) leaves nothing half done and the target goes to the
 * reference's own walk */
typedef struct {
    c4gpu_word_hit *hits;
    gint64 n_hits;
    gint frame;
    } ShimFrameHits;

static gboolean seed_scan_string(ShimSeedTab *st, gchar *seq, gint frame, ShimFrameHits *out){
    register gint n = strlen(seq), i;
    register guchar *sym = g_new(guchar, n + 1);
    register c4gpu_word_hit *hits = NULL;
    int64_t n_hits = 0, cap;
    gint64 t0 = g_get_monotonic_time();
    for(i = 0; i < n; i++)
        sym[i] = st->column[(guchar)seq[i]];
    if(st->host_index){
        register GArray *h = g_array_new(FALSE, FALSE, sizeof(c4gpu_word_hit));
        for(i = st->wordlen - 1; i < n; i++){
            guint64 code = 0;
            register gint w, word;
            gboolean ok = TRUE;
            for(w = 0; w < st->wordlen; w++){
                register guchar s = sym[i - st->wordlen + 1 + w];
                if(!s)
                    ok = FALSE;
                code = code * st->width + s;
                }
            if(!ok)
                continue;
            word = GPOINTER_TO_INT(g_hash_table_lookup(st->host_index, &code));
            if(word){
                register gint32 e;
                for(e = g_array_index(st->first, gint32, word - 1); e < g_array_index(st->first, gint32, word); e++){
                    c4gpu_word_hit x;
                    x.pos = i; x.emit = e;
                    g_array_append_val(h, x);
                    }
                }
            }
        n_hits = h->len;
        hits = (c4gpu_word_hit*)g_array_free(h, FALSE);
    } else {
        cap = 4096 + n / 8;
        for(;;){
            hits = g_new(c4gpu_word_hit, cap);
            if(c4gpu_seed_scan(shim_get_ctx(), st->tab, sym, n, hits, cap, &n_hits) != 0){
                g_warning("c4gpu: %s -- this target is scanned on the CPU", c4gpu_last_error());
                g_free(hits); g_free(sym);
                return FALSE;
                }
            if(n_hits <= cap)
                break;
            g_free(hits);
            cap = n_hits;
            }
        }
    sdst.scans++; sdst.symbols += n; sdst.hits += n_hits;
    sdst.scan_ms += (g_get_monotonic_time() - t0) / 1e3;
    out->hits = hits; out->n_hits = n_hits; out->frame = frame;
    g_free(sym);
    return TRUE;
    }

static void seed_deliver_frame(ShimSeedTab *st, Sequence *target, ShimFrameHits *fh, GArray *mine){
    register gint64 k;
    gint64 t0 = g_get_monotonic_time();
    for(k = 0; k < fh->n_hits; k++){
        register ShimEmit *e = &g_array_index(st->emits, ShimEmit, fh->hits[k].emit);
        register gint tpos = fh->frame ? (fh->hits[k].pos * 3) + fh->frame - 1 : fh->hits[k].pos;       /* seeder.c:657-660 */
        seed_deliver(st->seeder, target, e, tpos - e->loader->tpos_modifier, mine);
        }
    sdst.host_ms += (g_get_monotonic_time() - t0) / 1e3;
    g_free(fh->hits);
    fh->hits = NULL;
    return;
    }

/* ---- C4GPU_SEED_FUSED: scan to stored HSPs in one call ----
 * C4GPU_SEED_FUSED_OPT=1 (opt-in, beside it): the route also takes soft-masked alphabets and --seedrepeat > 1
 * (c4gpu_seed_extend_opt); without it such runs keep the scan and extension calls, as they did before that call existed */

/* once per table: one loader behind every emission, its HSP_Param one the seeding seam takes (hsp_eligible, c4gpu_hsp.c) */
static void seed_fused_look(ShimSeedTab *st){
    register Seeder *seeder = st->seeder;
    register GHashTable *index;
    register Seeder_Loader *loader = NULL;
    register guint k;
    register gboolean codon;
    st->fused_looked = TRUE;
    if(!st->emits->len)
        return;
    for(k = 0; k < st->emits->len; k++){
        register ShimEmit *e = &g_array_index(st->emits, ShimEmit, k);
        if(loader && (e->loader != loader))
            return;
        loader = e->loader;
        }
    if((!loader->hsp_param->use_horizon) || (shim_match_kind(loader->hsp_param->match->type, FALSE) < 0))
        return;
    /* --seedrepeat > 1: only where every seed has a horizon entry -- equal advances; protein against DNA keeps the other route
     * (c4gpu_seed_extend_opt refuses it: the reference leaves its horizon array there) */
    if((loader->hsp_param->seed_repeat > 1)
    && ((!shim_nonzero(C4GPU_SEED_FUSED_OPT)) || (loader->hsp_param->match->query->advance != loader->hsp_param->match->target->advance)))
        return;
    codon = (loader->hsp_param->match->type == Match_Type_CODON2CODON);
    index = g_hash_table_new(g_direct_hash, g_direct_equal);
    st->fused_query = g_new0(gchar*, seeder->query_info_list->len + 1);
    for(k = 0; k < seeder->query_info_list->len; k++){
        register Seeder_QueryInfo *query_info = seeder->query_info_list->pdata[k];
        g_hash_table_insert(index, query_info, GINT_TO_POINTER(k + 1));
        st->fused_query[k] = Sequence_get_str(query_info->query);
        /* (an annotated query of a codon loader: its sets keep the reference's function, hsp_match_kind in c4gpu_hsp.c) */
        if((codon && query_info->query->annotation) || (query_info->query->alphabet->is_soft_masked && !shim_nonzero(C4GPU_SEED_FUSED_OPT)))
            loader = NULL;
        }
    st->fused_emits = g_new(c4gpu_seed_emit, st->emits->len);
    for(k = 0; loader && (k < st->emits->len); k++){
        register ShimEmit *e = &g_array_index(st->emits, ShimEmit, k);
        register gint at = GPOINTER_TO_INT(g_hash_table_lookup(index, e->query_info));
        if(!at)
            loader = NULL;
        st->fused_emits[k].pair = at - 1;
        st->fused_emits[k].query_pos = e->query_pos;
        }
    g_hash_table_destroy(index);
    st->fused_loader = loader;
    return;
    }

static gboolean seed_fused_wanted(ShimSeedTab *st, Sequence *target){
    if((!shim_nonzero(C4GPU_SEED_FUSED)) || shim_has(C4GPU_SEED_CHECK) || shim_has(C4GPU_HSP_CHECK) || shim_has(C4GPU_HSP_OFF))
        return FALSE;
    if(!st->fused_looked)
        seed_fused_look(st);
    /* (a soft-masked target with the second switch: c4gpu_seed_extend_opt takes the alphabets' flags) */
    return st->fused_loader && (shim_nonzero(C4GPU_SEED_FUSED_OPT) || !target->alphabet->is_soft_masked);
    }

/* the kept list on the device: one c4gpu_seed_extend_opt call.  The pairs hand the residues over with their case
 * (Sequence_get_str, as the masked flush of c4gpu_hsp.c does); whether a lower-case letter masks is the alphabets' business. */
static gboolean seed_fused_device(ShimSeedTab *st, Sequence *target, gchar *tstr, guchar **sym, gint32 *n_sym, gint n_strs,
                                  c4gpu_seed_hsp **kept, c4gpu_seed_extend_stats *stats, gint64 *first_hit){
    register Seeder *seeder = st->seeder;
    register HSP_Param *param = st->fused_loader->hsp_param;
    register gint n_pairs = seeder->query_info_list->len, i;
    register c4gpu_pair *pairs;
    static const gint32 frame_offset[3] = {0, 1, 2};
    register gboolean translated = param->match->target->is_translated;
    register gboolean ok = FALSE;
    register gint mask_query = 0, mask_target = target->alphabet->is_soft_masked ? 1 : 0;
    gint64 cap = 1024;
    c4gpu_params params;
    if((!st->fused_sent) && (c4gpu_wordtab_set_emissions(st->tab, st->fused_emits, st->emits->len) != 0))
        return FALSE;
    st->fused_sent = TRUE;
    shim_hsp_params(&params);
    pairs = g_new0(c4gpu_pair, n_pairs + 1);
    for(i = 0; i < n_pairs; i++){
        register Seeder_QueryInfo *query_info = seeder->query_info_list->pdata[i];
        pairs[i].query = (const uint8_t*)st->fused_query[i]; pairs[i].query_len = query_info->query->len;
        pairs[i].target = (const uint8_t*)tstr;              pairs[i].target_len = target->len;
        if(query_info->query->alphabet->is_soft_masked)      /* (one alphabet for all queries of a run) */
            mask_query = 1;
        }
    for(i = 0; i < n_strs; i++)
        cap += n_sym[i] / 64;
    for(;;){
        *kept = g_new(c4gpu_seed_hsp, cap + 1);
        if(c4gpu_seed_extend_opt(shim_get_ctx(), st->tab, &params, shim_match_kind(param->match->type, FALSE), pairs, n_pairs,
                                 (const uint8_t *const *)sym, n_sym, n_strs, translated ? 3 : 1, frame_offset,
                                 st->fused_loader->tpos_modifier, param->seedlen, param->dropoff, param->threshold,
                                 mask_query, mask_target, param->seed_repeat, *kept, cap, stats) != 0)
            break;
        if(stats->n_kept <= cap){
            ok = TRUE;
            break;
            }
        g_free(*kept);
        cap = stats->n_kept;
        }
    if(ok && (c4gpu_seed_extend_first_hits(shim_get_ctx(), st->tab, first_hit, n_pairs) != 0))
        ok = FALSE;
    if(!ok){
        g_free(*kept);
        *kept = NULL;
        }
    g_free(pairs);
    return ok;
    }

/* C4GPU_SEED_HOST: the kept list from the reference's own HSPset_seed_hsp, one scratch set per query fed the host scan's seeds
 * in order; what it stores is read as it is stored (before any finalising, which may reorder the list).  The filter queues
 * (--hspfilter) are for the real set: the scratch sets run without them.  A seed without a horizon entry (negative section:
 * see hsp_replay, c4gpu_hsp.c) gets a scratch set of its own. */
static gboolean seed_fused_host(ShimSeedTab *st, Sequence *target, gchar **strs, gint *str_frame, gint n_strs,
                                c4gpu_seed_hsp **kept, c4gpu_seed_extend_stats *stats, gint64 *first_hit){
    register Seeder *seeder = st->seeder;
    register HSP_Param *param = st->fused_loader->hsp_param;
    register gint n_pairs = seeder->query_info_list->len, i, aq = param->match->query->advance, at = param->match->target->advance;
    register HSPset **scratch = g_new0(HSPset*, n_pairs + 1);
    register GArray *out = g_array_new(FALSE, FALSE, sizeof(c4gpu_seed_hsp));
    register gint keep_filter = param->has->filter_threshold;
    register gint64 k, walk = 0;
    ShimFrameHits fh;
    memset(stats, 0, sizeof(*stats));
    param->has->filter_threshold = 0;
    for(i = 0; i < n_strs; i++){
        if(!seed_scan_string(st, strs[i], str_frame[i], &fh))
            continue;                                               /* (the host scan does not fail) */
        for(k = 0; k < fh.n_hits; k++, walk++){
            register c4gpu_seed_emit *e = &st->fused_emits[fh.hits[k].emit];
            register Seeder_QueryInfo *query_info = seeder->query_info_list->pdata[e->pair];
            register gint tpos = (fh.frame ? (fh.hits[k].pos * 3) + fh.frame - 1 : fh.hits[k].pos) - st->fused_loader->tpos_modifier;
            register gint qlen = query_info->query->len, diag_pos = (tpos * aq) - (e->query_pos * at);
            /* a codon loader (aq 3): the reference's own unsigned sum and remainder (hspset.c:942-943), as c4gpu_seed_extend has it */
            register gint section_pos = (aq > 1) ? (gint)(((guint)diag_pos + (guint)qlen) % (guint)qlen) : (diag_pos + qlen) % qlen;
            register HSPset *set;
            register guint before;
            if(first_hit[e->pair] < 0)
                first_hit[e->pair] = walk;
            if(section_pos < 0)
                set = HSPset_create(query_info->query, target, param);
            else {
                if(!scratch[e->pair])
                    scratch[e->pair] = HSPset_create(query_info->query, target, param);
                set = scratch[e->pair];
                }
            before = set->hsp_list->len;
            if(section_pos < 0)
                stats->n_extended++;
            else if(param->seed_repeat > 1){
                /* the repeat rule as the set is about to apply it (hspset.c:950-970): another diagonal's tag clears the entry */
                register gboolean same = ((guint)set->horizon[2][section_pos][e->query_pos % aq][tpos % at]
                                          == ((guint)diag_pos + (guint)qlen));
                if(((!same) || (tpos >= set->horizon[0][section_pos][e->query_pos % aq][tpos % at]))
                && (((same ? set->horizon[1][section_pos][e->query_pos % aq][tpos % at] : 0) + 1) >= param->seed_repeat))
                    stats->n_extended++;
            } else if(tpos >= set->horizon[0][section_pos][e->query_pos % aq][tpos % at])
                stats->n_extended++;
            HSPset_seed_hsp_cpu(set, e->query_pos, tpos);
            if(set->hsp_list->len > before){
                register HSP *h = set->hsp_list->pdata[set->hsp_list->len - 1];
                c4gpu_seed_hsp x;
                x.seed = walk; x.pair = e->pair;
                x.hsp.query_start = h->query_start; x.hsp.target_start = h->target_start; x.hsp.length = h->length;
                x.hsp.score = h->score; x.hsp.cobs = h->cobs;
                g_array_append_val(out, x);
                }
            if(section_pos < 0)
                HSPset_destroy(set);
            }
        g_free(fh.hits);
        }
    param->has->filter_threshold = keep_filter;
    for(i = 0; i < n_pairs; i++)
        if(scratch[i])
            HSPset_destroy(scratch[i]);
    g_free(scratch);
    stats->n_hits = walk;
    stats->n_kept = out->len;
    stats->n_below = stats->n_extended - stats->n_kept;
    *kept = (c4gpu_seed_hsp*)g_array_free(out, FALSE);
    return TRUE;
    }

/* What seed_deliver does, for the HSPs that are kept.  The reference creates a query's Comparison at its first word hit, kept
 * or not (seeder.c:634-640), and reports in that order (seeder.c:899-913): the queries that keep an HSP get theirs here in the
 * order of their first hits, then every HSP goes to its set in walk order. */
static gint seed_fused_order(gconstpointer a, gconstpointer b, gpointer first_hit){
    register gint64 x = ((const gint64*)first_hit)[*(const gint*)a], y = ((const gint64*)first_hit)[*(const gint*)b];
    return (x < y) ? -1 : ((x > y) ? 1 : 0);
    }
static void seed_fused_deliver(ShimSeedTab *st, Sequence *target, const c4gpu_seed_hsp *kept, const c4gpu_seed_extend_stats *stats,
                               const gint64 *first_hit){
    register Seeder *seeder = st->seeder;
    register gint n_pairs = seeder->query_info_list->len, n_with = 0, i;
    register gint *with = g_new(gint, n_pairs + 1);
    register gboolean *has = g_new0(gboolean, n_pairs + 1);
    register gint64 k;
    for(k = 0; k < stats->n_kept; k++)
        if(!has[kept[k].pair]){
            has[kept[k].pair] = TRUE;
            with[n_with++] = kept[k].pair;
            }
    g_qsort_with_data(with, n_with, sizeof(gint), seed_fused_order, (gpointer)first_hit);
    for(i = 0; i < n_with; i++){
        register Seeder_QueryInfo *query_info = seeder->query_info_list->pdata[with[i]];
        if(!query_info->curr_comparison){
            query_info->curr_comparison = Comparison_create(seeder->comparison_param, query_info->query, target);
            g_ptr_array_add(seeder->active_queryinfo_list, query_info);
            }
        }
    g_free(with);
    g_free(has);
    for(k = 0; k < stats->n_kept; k++){
        register Seeder_QueryInfo *query_info = seeder->query_info_list->pdata[kept[k].pair];
        register HSPset *hspset;
        hspset = *(HSPset**)((gchar*)query_info->curr_comparison + st->fused_loader->hspset_offset);
        HSPset_add_known_hsp(hspset, kept[k].hsp.query_start, kept[k].hsp.target_start, kept[k].hsp.length);
        }
    seeder->comparison_count += stats->n_hits;
    return;
    }

/* TRUE: the target's HSPs are in their sets */
static gboolean seed_fused_target(ShimSeedTab *st, Sequence *target, gchar **strs, gint *str_frame, gint n_strs){
    c4gpu_seed_hsp *kept = NULL;
    c4gpu_seed_extend_stats stats;
    register gboolean ok;
    register gint i, n_pairs = st->seeder->query_info_list->len;
    register gint64 *first_hit = g_new(gint64, n_pairs + 1);
    gint64 t0 = g_get_monotonic_time();
    for(i = 0; i < n_pairs; i++)
        first_hit[i] = -1;
    if(st->host_index)
        ok = seed_fused_host(st, target, strs, str_frame, n_strs, &kept, &stats, first_hit);
    else {
        guchar *sym[3];
        gint32 n_sym[3];
        register gchar *tstr = Sequence_get_str(target);
        for(i = 0; i < n_strs; i++){
            register gint n = strlen(strs[i]), x;
            sym[i] = g_new(guchar, n + 1);
            for(x = 0; x < n; x++)
                sym[i][x] = st->column[(guchar)strs[i][x]];
            n_sym[i] = n;
            }
        ok = seed_fused_device(st, target, tstr, sym, n_sym, n_strs, &kept, &stats, first_hit);
        for(i = 0; i < n_strs; i++){
            g_free(sym[i]);
            if(ok){
                sdst.scans++; sdst.symbols += n_sym[i];
                }
            }
        if(ok)
            sdst.hits += stats.n_hits;
        g_free(tstr);
        if(!ok)
            g_warning("c4gpu: %s -- this target takes the scan and extension calls", c4gpu_last_error());
        }
    if(!ok){
        g_free(first_hit);
        return FALSE;
        }
    seed_fused_deliver(st, target, kept, &stats, first_hit);
    g_free(kept);
    g_free(first_hit);
    sdst.fused_targets++; sdst.fused_hits += stats.n_hits; sdst.fused_extended += stats.n_extended; sdst.fused_kept += stats.n_kept;
    sdst.fused_ms += (g_get_monotonic_time() - t0) / 1e3;
    return TRUE;
    }

void Seeder_add_target(Seeder *seeder, Sequence *target){
    register ShimSeedTab *st = NULL;
    register Match *match = seeder->any_hsp_param->match;
    register gint i;
    register Seeder_QueryInfo *query_info;
    register GArray *mine = NULL, *theirs = NULL;
    ShimFrameHits frames[3];
    gchar *strs[3];
    gint str_frame[3], n_strs = 0;
    gint n_frames = 0;
    gboolean ok = TRUE, fused = FALSE;
    register gboolean off = shim_has(C4GPU_SEED_OFF) || (shim_batch_size() <= 0);
    shim_mark("Seeder_add_target");
    /* a translated query (codon2codon: match advance 3 on the query) has a word list per query frame, all in one automaton, its
     * seeds' query positions already nucleotide positions (seeder.c:540-545): the reference's walk unless C4GPU_CODON_SEED=1 */
    if((!off) && ((match->query->advance == 1) || shim_nonzero(C4GPU_CODON_SEED)) && (shim_has(C4GPU_SEED_HOST) || shim_ctx_nowait())){
        st = seed_state(seeder);
        if(st->hopeless)
            st = NULL;
        else if(!st->usable){
            if(!seed_worth_it(st, target)){
                st->walked += target->len;
                sdst.cpu_targets++;
                st = NULL;
            } else if(!seed_build(st)){
                st->hopeless = TRUE;
                st = NULL;
                }
            }
        }
    shim_mark("word table ready");
    if(!st){
        Seeder_add_target_cpu(seeder, target);
        return;
        }
    if(shim_has(C4GPU_SEED_CHECK)){
        /* the reference's own walk first, its seeds written down instead of extended (no set becomes non-empty, so its
         * report loop finds nothing to report) */
        theirs = seed_record = g_array_new(FALSE, FALSE, sizeof(ShimSeedRec));
        Seeder_add_target_cpu(seeder, target);
        seed_record = NULL;
        mine = g_array_new(FALSE, FALSE, sizeof(ShimSeedRec));
        }
    sdst.targets++;
    Sequence_share(target);
    if(match->target->is_translated){                          /* seeder.c:868-884 */
        for(i = 0; i < 3; i++){
            register Sequence *aa_seq = Sequence_translate(target, match->mas->translate, i + 1);
            register Sequence *masked = Sequence_mask(aa_seq);
            strs[n_strs] = Sequence_get_str(masked);
            str_frame[n_strs++] = i + 1;
            Sequence_destroy(aa_seq);
            Sequence_destroy(masked);
            }
    } else {
        register Sequence *masked = Sequence_mask(target);
        strs[0] = Sequence_get_str(masked);
        str_frame[0] = 0;
        n_strs = 1;
        Sequence_destroy(masked);
        }
    if(seed_fused_wanted(st, target))
        fused = seed_fused_target(st, target, strs, str_frame, n_strs);
    for(i = 0; (i < n_strs) && ok && (!fused); i++){
        ok = seed_scan_string(st, strs[i], str_frame[i], &frames[n_frames]);
        if(ok)
            n_frames++;
        }
    for(i = 0; i < n_strs; i++)
        g_free(strs[i]);
    if(!ok){
        /* nothing has been delivered yet: this target (and the rest of this seeder's) keeps the reference's walk */
        for(i = 0; i < n_frames; i++)
            g_free(frames[i].hits);
        st->hopeless = TRUE;
        sdst.targets--;
        sdst.cpu_targets++;
        if(theirs){                                   /* check mode: the reference's walk has already run, its seeds only written down */
            g_array_free(theirs, TRUE);
            g_array_free(mine, TRUE);
            }
        Seeder_add_target_cpu(seeder, target);
        Sequence_destroy(target);
        return;
        }
    for(i = 0; i < n_frames; i++)
        seed_deliver_frame(st, target, &frames[i], mine);
    Sequence_destroy(target);
    if(theirs){
        if(theirs->len != mine->len)
            g_error("c4gpu seed check: the reference's walk finds %u seeds, the device scan %u", theirs->len, mine->len);
        for(i = 0; i < (gint)mine->len; i++){
            register ShimSeedRec *a = &g_array_index(theirs, ShimSeedRec, i), *b = &g_array_index(mine, ShimSeedRec, i);
            if((a->query != b->query) || (a->param != b->param) || (a->query_pos != b->query_pos) || (a->target_pos != b->target_pos))
                g_error("c4gpu seed check: seed %d differs: reference (%u, %u), device scan (%u, %u)", i, a->query_pos,
                        a->target_pos, b->query_pos, b->target_pos);
            }
        sdst.checked += mine->len;
        g_array_free(theirs, TRUE);
        g_array_free(mine, TRUE);
        }
    shim_mark("target scanned, seeds delivered");
    /* Report matches, seeder.c:899-913 */
    for(i = 0; i < (gint)seeder->active_queryinfo_list->len; i++){
        query_info = seeder->active_queryinfo_list->pdata[i];
        if(Comparison_has_hsps(query_info->curr_comparison)){
            Comparison_finalise(query_info->curr_comparison);
            seeder->report_func(query_info->curr_comparison, seeder->user_data);
            }
        Comparison_destroy(query_info->curr_comparison);
        query_info->curr_comparison = NULL;
        }
    g_ptr_array_set_size(seeder->active_queryinfo_list, 0);
    shim_mark("comparisons reported");
    return;
    }

/* a seeder's word table goes with it (analysis.c builds a new seeder for every --fsmmemory load of queries) */
void Seeder_destroy(Seeder *seeder){
    register ShimSeedTab *st = seed_tabs ? g_hash_table_lookup(seed_tabs, seeder) : NULL;
    if(st){
        g_hash_table_remove(seed_tabs, seeder);
        if(st->tab)
            c4gpu_wordtab_destroy(st->tab);
        if(st->host_index)
            g_hash_table_destroy(st->host_index);
        if(st->fused_query){
            register guint k;
            for(k = 0; st->fused_query[k]; k++)
                g_free(st->fused_query[k]);
            g_free(st->fused_query);
            }
        g_free(st->fused_emits);
        if(st->codes){
            g_array_free(st->codes, TRUE); g_array_free(st->first, TRUE); g_array_free(st->emits, TRUE);
            }
        g_free(st);
        }
    Seeder_destroy_cpu(seeder);
    return;
    }

void shim_seed_report(void){
    if(shim_has(C4GPU_VERBOSE) && sdst.cpu_targets)
        g_message("c4gpu seed: %ld targets left to the reference's walk (their seeder's word table was not worth reading yet)",
                  sdst.cpu_targets);
    if(shim_has(C4GPU_VERBOSE) && sdst.targets)
        g_message("c4gpu seed: %ld targets walked in %ld device scans (%ld symbols): %ld word hits; scans %.0f ms, "
                  "delivery %.0f ms, word tables (%ld words, %ld emissions) %.0f ms%s", sdst.targets, sdst.scans, sdst.symbols,
                  sdst.hits, sdst.scan_ms, sdst.host_ms, sdst.words, sdst.emits, sdst.table_ms,
                  sdst.checked ? "; every seed equal to the reference's own walk" : "");
    if(shim_has(C4GPU_VERBOSE) && (sdst.read || sdst.built))
        g_message("c4gpu seed: word tables: %ld read off the automaton, %ld built on the device (c4gpu_wordtab_build %.0f ms)",
                  sdst.read, sdst.built, sdst.build_ms);
    if(shim_has(C4GPU_VERBOSE) && shim_nonzero(C4GPU_SEED_FUSED))
        g_message("c4gpu seed fused: %ld targets through c4gpu_seed_extend: %ld word hits, %ld extensions, %ld HSPs kept "
                  "(%.0f ms with delivery)", sdst.fused_targets, sdst.fused_hits, sdst.fused_extended, sdst.fused_kept, sdst.fused_ms);
    return;
    }
