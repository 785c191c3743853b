/* c4gpu_shim.h — what the two files of the exonerate-gpu shim share (c4gpu_shim.c: the Viterbi plug-in table and
 * the exhaustive batching seam; c4gpu_bsdp.c: the heuristic / BSDP seam). */
#ifndef INCLUDED_C4GPU_SHIM_H
#define INCLUDED_C4GPU_SHIM_H

#include "c4.h"
#include "ungapped.h"
#include "optimal.h"
#include "gam.h"
#include "comparison.h"
#include "hspset.h"
#include "c4gpu.h"

c4gpu_ctx *shim_get_ctx(void);
const gchar *shim_env(const gchar *name);   /* a C4GPU_* variable as it was when the process started: never getenv (c4gpu_shim.c) */
gint shim_device_ordinal(void);        /* --gpudevice / C4GPU_DEVICE: for a second context of the same device */
c4gpu_ctx *shim_ctx_nowait(void);       /* NULL while the device is still being opened (small work does not wait) */
void shim_mark(const gchar *what);
gint shim_batch_size(void);
/* closed C4_Model -> c4gpu_model; allow_span: BSDP's span models (cell_start_func / cell_end_func become matrices) */
gboolean shim_flatten_any(C4_Model *m, Ungapped_Data *ud, c4gpu_model *out, gboolean allow_span);
/* ... for a seam that serves split codons against a translated DNA query (coding2genome) under a switch of its own, whatever
 * C4GPU_CODING2GENOME (the exhaustive seam's switch) says */
gboolean shim_flatten_split_codon(C4_Model *m, Ungapped_Data *ud, c4gpu_model *out);
/* ... and with BSDP's span models allowed (the BSDP seam, C4GPU_CODING2GENOME_BSDP=1) */
gboolean shim_flatten_split_codon_any(C4_Model *m, Ungapped_Data *ud, c4gpu_model *out, gboolean allow_span);
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
gboolean shim_codon_seed(void);        /* C4GPU_CODON_SEED=1: the HSP and word-scan seams take the translated models' seeds */
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
