/* c4gpu_shim.h — what the five files of the exonerate-gpu shim share (c4gpu_shim.c: the Viterbi plug-in table and the exhaustive
 * batching seam; c4gpu_bsdp.c: the heuristic / BSDP seam; c4gpu_sdp.c: the SDP seam; c4gpu_hsp.c: HSP extension; c4gpu_seed.c:
 * the word scan).  Their switches: c4gpu_switches.h. */
#ifndef INCLUDED_C4GPU_SHIM_H
#define INCLUDED_C4GPU_SHIM_H

#include "c4.h"
#include "ungapped.h"
#include "optimal.h"
#include "gam.h"
#include "comparison.h"
#include "hspset.h"
#include "c4gpu.h"
#include "c4gpu_switches.h"

c4gpu_ctx *shim_get_ctx(void);
gint shim_device_ordinal(void);        /* --gpudevice / C4GPU_DEVICE: for a second context of the same device */
c4gpu_ctx *shim_ctx_nowait(void);       /* NULL while the device is still being opened (small work does not wait) */
void shim_mark(const gchar *what);
gint shim_batch_size(void);
/* a seam's device part on a thread of its own: on unless its switch says 0 (C4GPU_ASYNC, C4GPU_SDP_ASYNC) */
static inline gboolean shim_async(ShimSwitchKey key){ return !shim_is(key, 0); }
/* closed C4_Model -> c4gpu_model.  What a seam lets through is its flag word, from one small function of the seam's own (the
 * table of seam x switch -> flags: c4gpu_switches.h); the flattening reads no switch itself. */
#define SHIM_FLATTEN_SPANS       1u    /* BSDP's span models: cell_start_func / cell_end_func become matrices (c4gpu_bsdp.c) */
#define SHIM_FLATTEN_ANNOTATED   2u    /* the seam hands a DNA query's annotation to the library (c4gpu_batch_set_annotation) */
#define SHIM_FLATTEN_SPLIT_CODON 4u    /* split codons against a translated DNA query (coding2genome and what is derived from it) */
gboolean shim_flatten(C4_Model *m, Ungapped_Data *ud, c4gpu_model *out, guint flags);
/* ... and the device family of the result, or -1 when the flattening declines (or the tables have no family) */
gint shim_model_family(C4_Model *m, Ungapped_Data *ud, guint flags, c4gpu_model *out);
/* "is this served", asked once per object: a pointer key -> not asked yet / no / yes (the table is made on first use) */
enum { SHIM_MEMO_UNKNOWN = 0, SHIM_MEMO_NO, SHIM_MEMO_YES };
gint shim_memo_get(GHashTable **memo, gconstpointer key);
gboolean shim_memo_put(GHashTable **memo, gconstpointer key, gboolean yes);      /* returns yes */
/* TRUE when some span of the model (C4_Model_add_span) loops on the query axis: the device SDP passes and BSDP's compiled span
 * families only know spans along the target (introns), so the heuristic seams leave such a model (ner: a span on both axes,
 * ner.c:105) to the reference's own functions */
gboolean shim_model_has_query_span(C4_Model *m);
/* a transition that advances the query by more than one row (coding2coding, ungapped:trans): served on the exhaustive seam and,
 * coding2coding, by BSDP's derived families; the other heuristic seams (HSP extension, seeding: C4GPU_CODON_SEED=1; SDP:
 * C4GPU_CODON_SDP=1 for coding2coding, C4GPU_CODING2GENOME_SDP=1 for coding2genome) leave such models to the reference unless
 * asked */
gboolean shim_model_has_wide_query_advance(C4_Model *m);
void shim_params(Ungapped_Data *ud, c4gpu_params *p);
/* scoring data for calls that have no model at hand (HSP seeding): Match_ArgumentSet's matrices and translation */
void shim_hsp_params(c4gpu_params *p);
/* c4gpu_hsp.c */
void shim_hsp_report(void);
/* the device's match kind, or -1; codons: with C4GPU_CODON_SEED, and not for an annotated query (the scan seam passes FALSE) */
gint shim_match_kind(Match_Type type, gboolean annotated_query);
/* c4gpu_bsdp.c */
void shim_bsdp_flush(void);
void shim_bsdp_report(void);
Alignment *shim_bsdp_find_path(Optimal *optimal, Region *region, SubOpt *subopt);
/* c4gpu_seed.c */
gboolean shim_seed_recording(HSPset *hsp_set, guint query_start, guint target_start);
void shim_seed_report(void);
/* c4gpu_sdp.c */
gboolean shim_sdp_collect(GAM *gam, Comparison *comparison);
gboolean shim_sdp_replaying(void);
gboolean shim_sdp_busy(void);
void shim_sdp_flush(void);
void shim_sdp_report(void);

#endif /* INCLUDED_C4GPU_SHIM_H */
