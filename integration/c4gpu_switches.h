/* c4gpu_switches.h — every C4GPU_* variable the drop-in's shim reads: one list, read once before main (shim_env_snapshot,
 * c4gpu_shim.c), asked by key ever after: an accessor is an array index, no getenv (it races with the setenv calls of the HIP
 * start-up on the device thread) and no string compare on any call path.  The accessors are those of the library's own table
 * (exonerate_amd/csrc/c4_config.h): has = the variable is there, whatever it says; num / real = its atoi / atof, or the
 * default; is = there AND equal to v; nonzero = there AND atoi != 0; text = the string itself, NULL when not there.
 * The truth rules differ from switch to switch and stay as they are: each key's comment gives its rule, its section the seam.
 *
 * Which switch lets what through the flattening (shim_flatten's flags, c4gpu_shim.h) -- seam x switch -> flags:
 *   seam (its flag function)                      always      C4GPU_CODING2GENOME == 1   the seam's own switch
 *   per call + exhaustive (shim_optimal_flags)    ANNOTATED   + SPLIT_CODON              (the same switch)
 *   SDP  (sdp_flatten_flags)                      -           + SPLIT_CODON              C4GPU_CODING2GENOME_SDP != 0: + SPLIT_CODON
 *   BSDP (bsdp_flatten_flags; SPANS per call)     -           + SPLIT_CODON              C4GPU_CODING2GENOME_BSDP == 1: + SPLIT_CODON
 * So C4GPU_CODING2GENOME, the exhaustive seam's switch, opens the split-codon calcs at EVERY seam's flattening (with it alone the
 * per-call path flattens coding2genome's derived models); which pairs a heuristic seam COLLECTS is its own switch's business
 * (sdp_wide_model_served, bsdp_wide_model_served), so a heuristic run with it alone stays with the reference. */
#ifndef INCLUDED_C4GPU_SWITCHES_H
#define INCLUDED_C4GPU_SWITCHES_H

#include <glib.h>

#define SHIM_SWITCHES(X) \
    /* ---- the process ---- */ \
    X(C4GPU_DISABLE)            /* has: no device at all, every call is the reference's */ \
    X(C4GPU_DEVICE)             /* num, default --gpudevice: the HIP device ordinal */ \
    X(C4GPU_VERBOSE)            /* has: the seams' report lines on stderr */ \
    X(C4GPU_TRACE)              /* has: shim_mark's wall-time marks (the library reads it too) */ \
    X(C4GPU_SEGV_TRACE)         /* has: a fatal signal writes the faulting thread's stack first */ \
    X(C4GPU_FAST_EXIT)          /* text begins with '1': leave with _exit */ \
    X(C4GPU_OWN_STREAM)         /* has: the context launches in a stream of its own */ \
    X(C4GPU_NO_WARM)            /* has: no code-object warm-up on the device thread */ \
    X(C4GPU_WAIT)               /* has: the seams in front of small work wait for the device too */ \
    /* ---- per call and the exhaustive seam (c4gpu_shim.c) ---- */ \
    X(C4GPU_CODING2GENOME)      /* == 1: coding2genome's exhaustive runs on the device; SPLIT_CODON at every seam (above) */ \
    X(C4GPU_MIN_CELLS)          /* real, default 1e5: single calls over fewer cells keep the CPU function */ \
    X(C4GPU_BATCH)              /* num, default --gpubatch: pairs per batch; <= 0 switches every batching seam off */ \
    X(C4GPU_BATCH_GB)           /* real, default 96: flush when the collected pairs would need more device memory */ \
    X(C4GPU_BATCH_ROUNDS)       /* num, default 4: sub-optimal rounds recorded per batch */ \
    X(C4GPU_ASYNC)              /* on unless == 0: a batch's device part on a thread of its own */ \
    X(C4GPU_SLOTS)              /* == 2: two resident batches taken in turn */ \
    X(C4GPU_EAGER)              /* nonzero: flush an eighth of a batch while the device is idle */ \
    X(C4GPU_KEEP_SUBOPT)        /* has: keep the SubOpt writes of a -S no replay */ \
    /* ---- the BSDP seam (c4gpu_bsdp.c) ---- */ \
    X(C4GPU_BSDP_OFF)           /* has: the seam is off */ \
    X(C4GPU_BSDP_HOST)          /* has: the batch computed by the reference's own DPs, no device asked */ \
    X(C4GPU_BSDP_CHECK)         /* == 1: every device candidate computed again by the reference and compared */ \
    X(C4GPU_REFINE_BATCH_OFF)   /* has: no refinement batch behind the sub-DPs */ \
    X(C4GPU_CODING2GENOME_BSDP) /* == 1: coding2genome's pairs collected; SPLIT_CODON at this seam */ \
    /* ---- the SDP seam (c4gpu_sdp.c) ---- */ \
    X(C4GPU_SDP_OFF)            /* has: the seam is off */ \
    X(C4GPU_SDP_HOST)           /* has: the batch computed by the reference's own SDP, no device asked */ \
    X(C4GPU_SDP_GB)             /* real, default from the device's memory: record budget of a flush */ \
    X(C4GPU_SDP_RESERVE)        /* real GB, default from the device's memory; there and <= 0: no arena reserved */ \
    X(C4GPU_SDP_ASYNC)          /* on unless == 0: flights on a thread and a context of their own */ \
    X(C4GPU_CODON_SDP)          /* nonzero: coding2coding's pairs collected */ \
    X(C4GPU_CODING2GENOME_SDP)  /* nonzero: coding2genome's pairs collected; SPLIT_CODON at this seam */ \
    /* ---- the HSP extension seam (c4gpu_hsp.c) ---- */ \
    X(C4GPU_HSP_OFF)            /* has: the seam is off (and with it the fused scan) */ \
    X(C4GPU_HSP_HOST)           /* has: the batch extended by the reference's own function, no device asked */ \
    X(C4GPU_HSP_CHECK)          /* has: every device HSP compared with the reference's; the fused scan is off */ \
    X(C4GPU_HSP_CHAIN)          /* on unless == 0: seeds of one diagonal chained on the device */ \
    X(C4GPU_HSP_DUMP)           /* text: a file the seam appends its seeds and HSPs to */ \
    X(C4GPU_CODON_SEED)         /* nonzero: the translated models' seeds, here and at the word scan */ \
    /* ---- the word-scan seam (c4gpu_seed.c) ---- */ \
    X(C4GPU_SEED_OFF)           /* has: the seam is off */ \
    X(C4GPU_SEED_HOST)          /* has: the scan by the reference's own walk, no device asked */ \
    X(C4GPU_SEED_CHECK)         /* has: every device scan compared with the reference's walk; the fused scan is off */ \
    X(C4GPU_SEED_FACTOR)        /* real, default 4: how much larger than the word table a target must be for the device */ \
    X(C4GPU_SEED_THREADS)       /* num, default min(8, cores): threads of the host's table build; there: at any size */ \
    X(C4GPU_SEED_COMPILE)       /* has: compile the reference's automaton as well */ \
    X(C4GPU_SEED_BUILD)         /* nonzero: the word table built on the device */ \
    X(C4GPU_SEED_BUILD_CHECK)   /* has: the device's table compared with the host's */ \
    X(C4GPU_SEED_FUSED)         /* nonzero: scan to stored HSPs in one device call */ \
    X(C4GPU_SEED_FUSED_OPT)     /* nonzero: the fused scan for soft-masked sets and --seedrepeat > 1 too */

typedef enum {
#define X(name) name,
    SHIM_SWITCHES(X)
#undef X
    SHIM_N_SWITCHES
} ShimSwitchKey;
#define SHIM_SWITCH_NAME(key) #key          /* the variable's name, for a message */

typedef struct { gboolean set; gint value; gdouble real; const gchar *text; } ShimSwitch;
extern ShimSwitch shim_switch[SHIM_N_SWITCHES];        /* c4gpu_shim.c; written before main, read-only ever after */

static inline gboolean shim_has(ShimSwitchKey k){ return shim_switch[k].set; }
static inline gint shim_num(ShimSwitchKey k, gint dflt){ return shim_switch[k].set ? shim_switch[k].value : dflt; }
static inline gdouble shim_real(ShimSwitchKey k, gdouble dflt){ return shim_switch[k].set ? shim_switch[k].real : dflt; }
static inline gboolean shim_is(ShimSwitchKey k, gint v){ return shim_switch[k].set && (shim_switch[k].value == v); }
static inline gboolean shim_nonzero(ShimSwitchKey k){ return shim_switch[k].set && (shim_switch[k].value != 0); }
static inline const gchar *shim_text(ShimSwitchKey k){ return shim_switch[k].text; }

#endif /* INCLUDED_C4GPU_SWITCHES_H */
