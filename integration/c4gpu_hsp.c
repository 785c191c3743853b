/* c4gpu_hsp.c — the seeding seam of the drop-in: the ungapped X-drop extensions of HSPset_seed_hsp
 * (src/comparison/hspset.c:933-997) of ALL word hits of a target scan in one device launch.  Third file of the
 * exonerate-gpu shim (integration/Makefile); INTEGRATION.md section 3b.
 *
 * The reference's word-neighbourhood FSM scan (seeder.c) reports word hits one by one to HSPset_seed_hsp, which tests
 * the diagonal's horizon, grows the HSP (trim, initial score, X-drop extension left and right) and stores it.  The
 * extension depends on the seed alone; only the horizon test, the threshold and the store order need the seeds in
 * sequence.  So the front of HSPset_seed_hsp only writes the seed down; at the first HSPset_finalise after a scan
 * (comparison.c:206-210) every pending seed of every HSPset goes to c4gpu_hsp_extend_batch, and each set is then
 * replayed in seed order: horizon test on the set's own horizon array (hspset.c:952-958), HSPset_add_known_hsp
 * (hspset.c:999: HSP_init + HSP_store, i.e. score, threshold, filter queues exactly as the reference) and the horizon
 * update.  The HSP lists that reach BSDP / SDP are the reference's, HSP for HSP.
 * Soft-masked sets (--softmaskquery / --softmasktarget) take the two-stage rule of hspset.c:981-995 on the device
 * (c4gpu_hsp_extend_batch_masked / _chains_masked): a seed whose masked extension stays below the threshold is DROPPED, the
 * replay stores nothing for it and moves the horizon to its masked end.
 * C4GPU_CODON_SEED=1 (opt-in): the codon sets of ungapped:trans and coding2coding are taken too (C4GPU_MATCH_CODON2CODON, both
 * advances 3, soft-masked ones included) -- but not a set whose query carries an annotation.
 * Not taken: --seedrepeat > 1, HSPsets without a horizon, match types other than DNA / protein / protein-vs-DNA (and, with the
 * switch, codon-vs-codon): those sets keep the reference's own function.
 * C4GPU_HSP_DUMP=FILE: every flushed set as one JSON line (hsp_dump_set).
 * C4GPU_HSP_HOST=1 (CPU test of the seam): the extensions come from the reference's own HSPset_seed_hsp on scratch sets.
 * C4GPU_HSP_CHECK=1: after the device call every extended seed is compared with that function's result (kept or dropped,
 * ends, score, masked end); the run aborts at the first difference. */
#include <string.h>
#include <stdlib.h>

#include "hspset.h"
#include "match.h"
#include "sequence.h"

#include "c4gpu.h"
#include "c4gpu_shim.h"

extern void HSPset_seed_hsp_cpu(HSPset *hsp_set, guint query_start, guint target_start);
extern HSPset *HSPset_finalise_cpu(HSPset *hsp_set);

typedef struct { HSPset *set; GArray *seeds; /* guint pairs (query_start, target_start) */ } ShimSeedSet;

static GHashTable *hsp_pending = NULL;          /* HSPset* -> ShimSeedSet* */
static GPtrArray *hsp_order = NULL;             /* ShimSeedSet*, in order of first seed */
static struct { long sets, seeds, stored, dropped, checked, flushes; double device_ms; } hst;

gint shim_match_kind(Match_Type type, gboolean annotated_query){
    switch(type){
        case Match_Type_DNA2DNA: return C4GPU_MATCH_DNA2DNA;
        case Match_Type_PROTEIN2PROTEIN: return C4GPU_MATCH_PROTEIN2PROTEIN;
        case Match_Type_PROTEIN2DNA: return C4GPU_MATCH_PROTEIN2DNA;
        /* C4GPU_CODON_SEED (opt-in): the seeds of the translated models (ungapped:trans, coding2coding) are taken too; a query
         * with an annotation keeps the reference's function, which vetoes codons outside the CDS frame inside the score
         * (Match_3_3_split_score_func, match.c:513-519) */
        case Match_Type_CODON2CODON: return (shim_nonzero(C4GPU_CODON_SEED) && !annotated_query) ? C4GPU_MATCH_CODON2CODON : -1;
        default: return -1;
        }
    }

static gint hsp_match_kind(HSPset *hsp_set){
    return shim_match_kind(hsp_set->param->match->type, hsp_set->query->annotation != NULL);
    }

static const gchar *hsp_match_name(HSPset *hsp_set){
    switch(hsp_set->param->match->type){
        case Match_Type_DNA2DNA: return "dna2dna";
        case Match_Type_PROTEIN2PROTEIN: return "protein2protein";
        case Match_Type_PROTEIN2DNA: return "protein2dna";
        case Match_Type_CODON2CODON: return "codon2codon";
        default: return "other";
        }
    }

/* hspset.c:935-943 as the reference computes it: Sequence.len is a guint, so the sum and the remainder are unsigned */
static gint hsp_section(HSPset *hsp_set, guint query_start, guint target_start){
    register gint diag_pos = (target_start * hsp_set->param->match->query->advance)
                           - (query_start * hsp_set->param->match->target->advance);
    return (diag_pos + hsp_set->query->len) % hsp_set->query->len;
    }

static gboolean hsp_eligible(HSPset *hsp_set){
    if(shim_has(C4GPU_HSP_OFF) || (!hsp_set->horizon) || (hsp_set->param->seed_repeat > 1) || (hsp_match_kind(hsp_set) < 0))
        return FALSE;
    if(shim_batch_size() <= 0)
        return FALSE;
    /* a set the reference's own function has already stored an HSP in (its first word hits came while the device was still
     * being opened, shim_ctx_nowait) stays with that function: the replay starts from an empty set */
    if(!hsp_set->is_empty)
        return FALSE;
    return shim_has(C4GPU_HSP_HOST) || (shim_ctx_nowait() != NULL);
    }

void HSPset_seed_hsp(HSPset *hsp_set, guint query_start, guint target_start){
    register ShimSeedSet *ss;
    guint seed[2];
    if(shim_seed_recording(hsp_set, query_start, target_start))        /* C4GPU_SEED_CHECK: the reference's own walk, written down */
        return;
    ss = hsp_pending ? g_hash_table_lookup(hsp_pending, hsp_set) : NULL;
    if(!ss){
        if(!hsp_eligible(hsp_set)){
            HSPset_seed_hsp_cpu(hsp_set, query_start, target_start);
            return;
            }
        if(!hsp_pending){
            hsp_pending = g_hash_table_new(g_direct_hash, g_direct_equal);
            hsp_order = g_ptr_array_new();
            }
        ss = g_new0(ShimSeedSet, 1);
        ss->set = hsp_set;
        ss->seeds = g_array_new(FALSE, FALSE, 2 * sizeof(guint));
        g_hash_table_insert(hsp_pending, hsp_set, ss);
        g_ptr_array_add(hsp_order, ss);
        /* the seeder asks Comparison_has_hsps BEFORE it finalises (seeder.c:903-909): a set with pending word hits must
         * not look empty there; the replay sets the flag to what the reference would hold, and both consumers of a
         * reported comparison ask again (gam.c:740,1122) */
        hsp_set->is_empty = FALSE;
        }
    seed[0] = query_start; seed[1] = target_start;
    g_array_append_val(ss->seeds, seed);
    return;
    }

/* The mask functions are always set (match.c:670,679) and ask the sequence's alphabet: without --softmaskquery /
 * --softmasktarget nothing is ever masked, the masked first extension (hspset.c:981-990) is then the plain one, a second
 * extension from its ends finds what the first one found, and the threshold can wait for HSP_store.  Only a set with a
 * soft-masked alphabet needs the two stages. */
static gboolean hsp_set_masked(HSPset *hsp_set){
    return hsp_set->query->alphabet->is_soft_masked || hsp_set->target->alphabet->is_soft_masked;
    }

/* The reference's own answer for one seed, on a scratch HSPset (nothing in its way).  A plain set stores whatever grows
 * (threshold -1: the replay applies the real one); a soft-masked set runs with its real threshold, because the masked stage
 * compares with it: dropped = the scratch set stayed empty, and its horizon entry is the masked end (hspset.c:985-989),
 * handed back as (target_start = that end, length = 0). */
static void hsp_host_one(HSPset *hsp_set, guint query_start, guint target_start, c4gpu_hsp *out, gint32 *dropped){
    register gboolean masked = hsp_set_masked(hsp_set);
    register C4_Score keep = hsp_set->param->threshold;
    register HSPset *one;
    if(!masked)
        hsp_set->param->threshold = -1;
    one = HSPset_create(hsp_set->query, hsp_set->target, hsp_set->param);
    HSPset_seed_hsp_cpu(one, query_start, target_start);
    HSPset_finalise_cpu(one);
    if(one->hsp_list->len){
        register HSP *h = one->hsp_list->pdata[0];
        out->query_start = h->query_start; out->target_start = h->target_start;
        out->length = h->length; out->score = h->score; out->cobs = h->cobs;
        *dropped = 0;
    } else {
        register gint aq = hsp_set->param->match->query->advance, at = hsp_set->param->match->target->advance;
        register gint diag_pos = (target_start * aq) - (query_start * at);
        register gint section_pos = (diag_pos + hsp_set->query->len) % hsp_set->query->len;
        out->query_start = 0; out->length = 0; out->score = 0; out->cobs = 0;
        out->target_start = (section_pos >= 0) ? one->horizon[0][section_pos][query_start % aq][target_start % at] : 0;
        *dropped = 1;
        }
    HSPset_destroy(one);
    hsp_set->param->threshold = keep;
    return;
    }

/* C4GPU_HSP_CHECK: every seed the device extended against the reference's own function */
static void hsp_check(ShimSeedSet *ss, const c4gpu_hsp *hsp, const gint32 *dropped){
    register HSPset *hsp_set = ss->set;
    register gint aq = hsp_set->param->match->query->advance, at = hsp_set->param->match->target->advance;
    register guint k;
    for(k = 0; k < ss->seeds->len; k++){
        register guint *seed = &g_array_index(ss->seeds, guint, 2 * k);
        register gint diag_pos = (seed[1] * aq) - (seed[0] * at);
        register gint section_pos = (diag_pos + hsp_set->query->len) % hsp_set->query->len;
        c4gpu_hsp ref;
        gint32 ref_dropped;
        register gboolean same;
        if(hsp[k].length < 0)                                            /* skipped under its chain's horizon */
            continue;
        hsp_host_one(hsp_set, seed[0], seed[1], &ref, &ref_dropped);
        if(ref_dropped != dropped[k])
            same = FALSE;
        else if(ref_dropped)
            same = (section_pos < 0) || (ref.target_start == hsp[k].target_start + hsp[k].length * at);
        else
            same = (ref.query_start == hsp[k].query_start) && (ref.target_start == hsp[k].target_start)
                && (ref.length == hsp[k].length) && (ref.score == hsp[k].score);
        if(!same)
            g_error(SHIM_SWITCH_NAME(C4GPU_HSP_CHECK) ": seed (%u, %u) of [%s] vs [%s]: device %s (%d, %d, %d, score %d), reference %s (%d, %d, %d, score %d)",
                    seed[0], seed[1], hsp_set->query->id, hsp_set->target->id,
                    dropped[k] ? "dropped" : "kept", hsp[k].query_start, hsp[k].target_start, hsp[k].length, hsp[k].score,
                    ref_dropped ? "dropped, masked end" : "kept", ref.query_start, ref.target_start, ref.length, ref.score);
        hst.checked++;
        }
    return;
    }

/* the replay of one set: hspset.c:936-958 (seed_repeat == 1) around the precomputed HSPs; a dropped seed (soft-masked
 * sets, hspset.c:985-989) stores nothing and moves the horizon to its masked end */
static void hsp_replay(ShimSeedSet *ss, const c4gpu_hsp *hsp, const gint32 *dropped){
    register HSPset *hsp_set = ss->set;
    register gint aq = hsp_set->param->match->query->advance, at = hsp_set->param->match->target->advance;
    register guint k;
    hsp_set->is_empty = TRUE;                                            /* HSP_store clears it with the first HSP kept */
    for(k = 0; k < ss->seeds->len; k++){
        register guint *seed = &g_array_index(ss->seeds, guint, 2 * k);
        register gint diag_pos = (seed[1] * aq) - (seed[0] * at);
        register gint query_frame = seed[0] % aq, target_frame = seed[1] % at;
        register gint section_pos = (diag_pos + hsp_set->query->len) % hsp_set->query->len;
        /* a seed more than a query length above the main diagonal (query_start * target advance > target_start + query
         * length: protein2dna hits at the very start of a target) has a NEGATIVE section_pos in the reference
         * (hspset.c:943-944, its g_assert compiled out): an out-of-bounds horizon entry there, none here */
        register gint *horizon = (section_pos >= 0) ? &hsp_set->horizon[0][section_pos][query_frame][target_frame] : NULL;
        if(horizon && ((gint)seed[1] < *horizon))
            continue;
        if(dropped[k]){
            if(horizon)
                *horizon = hsp[k].target_start + hsp[k].length * at;     /* HSP_target_end of the masked-extended nascent HSP */
            hst.dropped++;
            continue;
            }
        HSPset_add_known_hsp(hsp_set, hsp[k].query_start, hsp[k].target_start, hsp[k].length);
        if(horizon)
            *horizon = hsp[k].target_start + hsp[k].length * at;         /* HSP_target_end */
        hst.stored++;
        }
    return;
    }

/* C4GPU_HSP_DUMP=FILE: one JSON line per set and flush -- what the set was given, what the reference's own function makes of
 * every seed by itself (hsp_host_one: [query_start, target_start, length, score, cobs, dropped]; a dropped seed carries its
 * masked end as target_start and length 0), and the HSPs the set holds after the replay (before it is finalised: with
 * --hspfilter they wait in the filter queues and are not listed).  tools/make_codon_hsp_golden.py turns it into fixtures. */
static void hsp_dump_str(FILE *fp, const gchar *s){
    fputc('"', fp);
    for(; *s; s++)
        if((*s != '"') && (*s != '\\') && ((guchar)*s >= 0x20))
            fputc(*s, fp);
    fputc('"', fp);
    return;
    }

static void hsp_dump_set(ShimSeedSet *ss, const gchar *qstr, const gchar *tstr){
    static FILE *fp = NULL;
    register HSPset *set = ss->set;
    register guint k;
    if(!fp && !(fp = fopen(shim_text(C4GPU_HSP_DUMP), "a")))
        g_error(SHIM_SWITCH_NAME(C4GPU_HSP_DUMP) ": cannot open [%s]", shim_text(C4GPU_HSP_DUMP));
    fprintf(fp, "{\"query_id\":");
    hsp_dump_str(fp, set->query->id);
    fprintf(fp, ",\"target_id\":");
    hsp_dump_str(fp, set->target->id);
    fprintf(fp, ",\"match\":\"%s\",\"seedlen\":%d,\"dropoff\":%d,\"threshold\":%d,\"query_advance\":%d,\"target_advance\":%d,"
                "\"seed_repeat\":%d,\"mask_query\":%s,\"mask_target\":%s,\"query\":", hsp_match_name(set), (gint)set->param->seedlen,
            (gint)set->param->dropoff, (gint)set->param->threshold, (gint)set->param->match->query->advance,
            (gint)set->param->match->target->advance, (gint)set->param->seed_repeat,
            set->query->alphabet->is_soft_masked ? "true" : "false", set->target->alphabet->is_soft_masked ? "true" : "false");
    hsp_dump_str(fp, qstr);
    fprintf(fp, ",\"target\":");
    hsp_dump_str(fp, tstr);
    fprintf(fp, ",\"seeds\":[");
    for(k = 0; k < ss->seeds->len; k++)
        fprintf(fp, "%s[%u,%u]", k ? "," : "", g_array_index(ss->seeds, guint, 2 * k), g_array_index(ss->seeds, guint, 2 * k + 1));
    fprintf(fp, "],\"single\":[");
    for(k = 0; k < ss->seeds->len; k++){
        c4gpu_hsp h;
        gint32 d;
        hsp_host_one(set, g_array_index(ss->seeds, guint, 2 * k), g_array_index(ss->seeds, guint, 2 * k + 1), &h, &d);
        fprintf(fp, "%s[%d,%d,%d,%d,%d,%d]", k ? "," : "", h.query_start, h.target_start, h.length, h.score, h.cobs, d);
        }
    fprintf(fp, "],\"set\":[");
    for(k = 0; k < set->hsp_list->len; k++){
        register HSP *h = set->hsp_list->pdata[k];
        fprintf(fp, "%s[%u,%u,%u,%d,%u]", k ? "," : "", h->query_start, h->target_start, h->length, (gint)h->score, h->cobs);
        }
    fprintf(fp, "]}\n");
    fflush(fp);
    return;
    }

static void hsp_flush(void){
    register guint i, k, n_sets = hsp_order ? hsp_order->len : 0, total = 0;
    register GHashTable *seq_index;
    register GPtrArray *strs;
    c4gpu_pair *pairs;
    c4gpu_hsp_seed *seeds;
    c4gpu_hsp *hsps;
    gint *set_pair, *set_first;
    gint32 *chain_of = NULL, *horizon0 = NULL, *gc = NULL, *dropped;
    gint n_chains = 0;
    gboolean ok = TRUE;
    gint64 t0 = g_get_monotonic_time();
    if(!n_sets)
        return;
    for(i = 0; i < n_sets; i++)
        total += ((ShimSeedSet*)hsp_order->pdata[i])->seeds->len;
    pairs = g_new0(c4gpu_pair, n_sets);
    seeds = g_new(c4gpu_hsp_seed, total + 1);
    hsps = g_new0(c4gpu_hsp, total + 1);
    dropped = g_new0(gint32, total + 1);
    set_pair = g_new(gint, n_sets);
    set_first = g_new(gint, n_sets + 1);
    seq_index = g_hash_table_new(g_direct_hash, g_direct_equal);
    strs = g_ptr_array_new();
    for(i = 0, total = 0; i < n_sets; i++){
        register ShimSeedSet *ss = hsp_order->pdata[i];
        register gchar *qs, *ts;
        if(!(qs = g_hash_table_lookup(seq_index, ss->set->query))){
            qs = Sequence_get_str(ss->set->query);
            g_hash_table_insert(seq_index, ss->set->query, qs);
            g_ptr_array_add(strs, qs);
            }
        if(!(ts = g_hash_table_lookup(seq_index, ss->set->target))){
            ts = Sequence_get_str(ss->set->target);
            g_hash_table_insert(seq_index, ss->set->target, ts);
            g_ptr_array_add(strs, ts);
            }
        pairs[i].query = (const uint8_t*)qs;  pairs[i].query_len = ss->set->query->len;
        pairs[i].target = (const uint8_t*)ts; pairs[i].target_len = ss->set->target->len;
        set_first[i] = total;
        for(k = 0; k < ss->seeds->len; k++){
            seeds[total].pair = i;
            seeds[total].query_start = g_array_index(ss->seeds, guint, 2 * k);
            seeds[total].target_start = g_array_index(ss->seeds, guint, 2 * k + 1);
            total++;
            }
        }
    set_first[n_sets] = total;
    /* the horizon entry every seed is tested against (hspset.c:939-958): one chain per (set, section, frames); on the
     * device a chain's seeds are taken in order and the ones below the running horizon are not extended at all
     * (c4gpu_hsp_extend_chains): a long identical diagonal costs one extension instead of one per word hit.
     * C4GPU_HSP_CHAIN=0: every seed is extended and the replay alone applies the horizon */
    if(!shim_has(C4GPU_HSP_HOST) && !shim_is(C4GPU_HSP_CHAIN, 0)){
        register GArray *h0 = g_array_new(FALSE, FALSE, sizeof(gint32));
        chain_of = g_new(gint32, total + 1);
        for(i = 0; i < n_sets; i++){
            register ShimSeedSet *ss = hsp_order->pdata[i];
            register HSPset *set = ss->set;
            register gint aq = set->param->match->query->advance, at = set->param->match->target->advance;
            register gint qlen = set->query->len, slots = qlen * aq * at, x;
            register gint32 *slot = g_new(gint32, slots > 0 ? slots : 1);
            for(x = 0; x < slots; x++)
                slot[x] = -1;
            for(k = 0; k < ss->seeds->len; k++){
                register guint *seed = &g_array_index(ss->seeds, guint, 2 * k);
                register gint diag_pos = (seed[1] * aq) - (seed[0] * at);
                register gint qf = seed[0] % aq, tf = seed[1] % at;
                /* (a codon set's wrapped seeds -- the common case there -- are on the entry the replay will find them on) */
                register gint section_pos = (aq > 1) ? hsp_section(set, seed[0], seed[1]) : (diag_pos + qlen) % qlen;
                gint32 h;
                if(section_pos < 0){                          /* no horizon entry (see hsp_replay): never skipped */
                    h = G_MININT32;
                    chain_of[set_first[i] + k] = h0->len;
                    g_array_append_val(h0, h);
                    continue;
                    }
                x = (section_pos * aq + qf) * at + tf;
                if(slot[x] < 0){
                    slot[x] = h0->len;
                    h = set->horizon[0][section_pos][qf][tf];
                    g_array_append_val(h0, h);
                    }
                chain_of[set_first[i] + k] = slot[x];
                }
            g_free(slot);
            }
        n_chains = h0->len;
        horizon0 = (gint32*)g_array_free(h0, FALSE);
        }
    if(shim_has(C4GPU_HSP_HOST)){
        /* the reference's own extension, one scratch HSPset per seed (hsp_host_one) */
        for(i = 0; i < n_sets; i++){
            register ShimSeedSet *ss = hsp_order->pdata[i];
            for(k = 0; k < ss->seeds->len; k++)
                hsp_host_one(ss->set, seeds[set_first[i] + k].query_start, seeds[set_first[i] + k].target_start,
                             hsps + set_first[i] + k, dropped + set_first[i] + k);
            }
    } else {
        /* one launch per (match type, seed length, dropoff, threshold, the two mask flags): in practice one or two per scan */
#define HSP_SAME_GROUP(a, b) ((hsp_match_kind((a)->set) == hsp_match_kind((b)->set)) \
                           && ((a)->set->param->seedlen == (b)->set->param->seedlen) \
                           && ((a)->set->param->dropoff == (b)->set->param->dropoff) \
                           && ((a)->set->param->threshold == (b)->set->param->threshold) \
                           && ((a)->set->query->alphabet->is_soft_masked == (b)->set->query->alphabet->is_soft_masked) \
                           && ((a)->set->target->alphabet->is_soft_masked == (b)->set->target->alphabet->is_soft_masked))
        gboolean *done = g_new0(gboolean, n_sets);
        c4gpu_params params;
        shim_hsp_params(&params);
        for(i = 0; ok && (i < n_sets); i++){
            register ShimSeedSet *si = hsp_order->pdata[i];
            register gint kind = hsp_match_kind(si->set), first = -1, count = 0;
            c4gpu_hsp_seed *gs;
            c4gpu_hsp *go;
            gint32 *gd;
            register gint mq = si->set->query->alphabet->is_soft_masked ? 1 : 0, mt = si->set->target->alphabet->is_soft_masked ? 1 : 0;
            if(done[i])
                continue;
            gs = g_new(c4gpu_hsp_seed, total + 1);
            go = g_new(c4gpu_hsp, total + 1);
            gd = g_new0(gint32, total + 1);
            gc = chain_of ? g_new(gint32, total + 1) : NULL;
            for(k = i; k < n_sets; k++){
                register ShimSeedSet *sk = hsp_order->pdata[k];
                if(done[k] || !HSP_SAME_GROUP(sk, si))
                    continue;
                done[k] = TRUE;
                memcpy(gs + count, seeds + set_first[k], sizeof(c4gpu_hsp_seed) * (set_first[k+1] - set_first[k]));
                if(gc)
                    memcpy(gc + count, chain_of + set_first[k], sizeof(gint32) * (set_first[k+1] - set_first[k]));
                count += set_first[k+1] - set_first[k];
                (void)first;
                }
            if(mq || mt){                                   /* the two-stage rule; runs without soft-masking keep the old calls */
                if((gc ? c4gpu_hsp_extend_chains_masked(shim_get_ctx(), &params, kind, pairs, n_sets, si->set->param->seedlen,
                                                        si->set->param->dropoff, mq, mt, si->set->param->threshold, gs, count,
                                                        gc, n_chains, horizon0, go, gd)
                       : c4gpu_hsp_extend_batch_masked(shim_get_ctx(), &params, kind, pairs, n_sets, si->set->param->seedlen,
                                                       si->set->param->dropoff, mq, mt, si->set->param->threshold, gs, count,
                                                       go, gd)) != 0)
                    ok = FALSE;
            } else if(gc){
                if(c4gpu_hsp_extend_chains(shim_get_ctx(), &params, kind, pairs, n_sets, si->set->param->seedlen,
                                           si->set->param->dropoff, gs, count, gc, n_chains, horizon0, go) != 0)
                    ok = FALSE;
            } else if(c4gpu_hsp_extend_batch(shim_get_ctx(), &params, kind, pairs, n_sets, si->set->param->seedlen,
                                      si->set->param->dropoff, gs, count, go) != 0)
                ok = FALSE;
            for(k = i, count = 0; ok && (k < n_sets); k++){            /* scatter back in the same order */
                register ShimSeedSet *sk = hsp_order->pdata[k];
                if(!HSP_SAME_GROUP(sk, si))
                    continue;
                memcpy(hsps + set_first[k], go + count, sizeof(c4gpu_hsp) * (set_first[k+1] - set_first[k]));
                memcpy(dropped + set_first[k], gd + count, sizeof(gint32) * (set_first[k+1] - set_first[k]));
                count += set_first[k+1] - set_first[k];
                }
            g_free(gs); g_free(go); g_free(gc); g_free(gd);
            }
#undef HSP_SAME_GROUP
        g_free(done);
        if(ok && shim_has(C4GPU_HSP_CHECK))
            for(i = 0; i < n_sets; i++)
                hsp_check(hsp_order->pdata[i], hsps + set_first[i], dropped + set_first[i]);
        }
    for(i = 0; i < n_sets; i++){
        register ShimSeedSet *ss = hsp_order->pdata[i];
        if(ok){
            hsp_replay(ss, hsps + set_first[i], dropped + set_first[i]);
        } else {                                             /* the device refused (e.g. a residue outside the alphabet) */
            ss->set->is_empty = TRUE;
            for(k = 0; k < ss->seeds->len; k++)
                HSPset_seed_hsp_cpu(ss->set, g_array_index(ss->seeds, guint, 2 * k), g_array_index(ss->seeds, guint, 2 * k + 1));
            }
        if(shim_has(C4GPU_HSP_DUMP))
            hsp_dump_set(ss, g_hash_table_lookup(seq_index, ss->set->query), g_hash_table_lookup(seq_index, ss->set->target));
        hst.sets++; hst.seeds += ss->seeds->len;
        g_array_free(ss->seeds, TRUE);
        g_free(ss);
        }
    if(!ok)
        g_warning("c4gpu: %s -- HSP extensions of this scan on the CPU", c4gpu_last_error());
    g_ptr_array_set_size(hsp_order, 0);
    g_hash_table_remove_all(hsp_pending);
    for(i = 0; i < strs->len; i++)
        g_free(strs->pdata[i]);
    g_ptr_array_free(strs, TRUE);
    g_hash_table_destroy(seq_index);
    g_free(pairs); g_free(seeds); g_free(hsps); g_free(dropped); g_free(set_pair); g_free(set_first); g_free(chain_of); g_free(horizon0);
    hst.flushes++;
    hst.device_ms += (g_get_monotonic_time() - t0) / 1e3;
    return;
    }

HSPset *HSPset_finalise(HSPset *hsp_set){
    if(hsp_order && hsp_order->len)
        hsp_flush();                 /* every set of this scan at once: the others are finalised right after */
    return HSPset_finalise_cpu(hsp_set);
    }

void shim_hsp_report(void){
    if(shim_has(C4GPU_VERBOSE) && hst.sets)
        g_message("c4gpu hsp: %ld word hits of %ld HSP sets extended in %ld device batch(es) (%.0f ms incl. flattening and "
                  "replay), %ld HSPs passed their horizon, %ld seeds dropped at masked ends, %ld checked against the reference",
                  hst.seeds, hst.sets, hst.flushes, hst.device_ms, hst.stored, hst.dropped, hst.checked);
    return;
    }
