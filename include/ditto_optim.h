/* ditto_optim.h — C-ABI of the fused training optimizer of libditto_hip.so (csrc/optim.hip): AdamW with gradient clipping by
 * global norm, an on-device skip of a step whose gradient norm is not finite, and an exponential moving average (EMA) of the
 * weights, over any number of separate fp32 tensors in at most three launches.
 *
 * The reference trains with torch.optim.AdamW alone (src/TrainDiTTO.py:52, src/utils/Trainer.py:69); it has no clipping and no
 * EMA.  The arithmetic here is torch's: torch.nn.utils.clip_grad_norm_ (norm_type 2), torch.optim.AdamW (decoupled decay, no
 * amsgrad), Tensor.lerp_ for the average.  The entries live in their own header, beside include/ditto_hip.h and under its
 * conventions (status codes, ditto_last_error, device pointers owned by the caller, no allocation, no synchronisation, one
 * stream-ordered enqueue per launch); DITTO_ABI_VERSION does not change with them.
 *
 * One step on a table of n_seg segments (one per parameter tensor):
 *   norm      = sqrt(sum over every segment of g^2)                      fp64 sums in a fixed order, see below
 *   clip      = min(1, max_norm / (norm + 1e-6))                          exactly 1 when max_norm <= 0 (clipping off)
 *   skip      = skip_nonfinite && !(norm is finite)                       a skipped step writes no tensor and advances nothing
 *   per element, fp32, gs = g * clip:
 *     pd   = p * fl(1 - lr wd)
 *     m'   = fmaf(fl(beta1), m, fl(1 - beta1) * gs)
 *     v'   = fmaf(fl(beta2), v, fl(1 - beta2) * (gs * gs))
 *     p'   = fmaf(-fl(lr / bc1), m' / fmaf(sqrtf(v'), fl(1 / sqrt(bc2)), fl(eps)), pd)      bc_k = 1 - beta_k^t, t the new step count
 *     ema' = fmaf(fl(1 - ema_decay), p' - ema, ema)                       where the segment has an ema
 *   fl() = one rounding of an fp64 value to fp32; the division is the correctly rounded one, the square root within 1 ulp; nothing is
 *   contracted.  tests/optim_ref.py derives its bounds from this expression.
 *
 * Chunks.  Segment s is cut into chunks of DITTO_OPTIM_CHUNK_QUADS 16-byte quads of ITS OWN elements (the last one shorter);
 * ditto_optim_seg.slot0 is the number of chunks of the segments in front of it, so chunk c of the table is chunk c - slot0 of the
 * last segment with slot0 <= c, and n_chunks = slot0 + chunks of the last segment.  Every kernel runs over this flat chunk list
 * (a workgroup strides over chunk indices when the grid is smaller).  The norm is the sum of one fp64 partial per chunk — lane
 * order, a fixed xor butterfly, the waves in index order — added in an order that depends on n_chunks only: its bits are a function
 * of the table and the gradients, not of the grid.
 */
#ifndef DITTO_OPTIM_H
#define DITTO_OPTIM_H

#include "ditto_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DITTO_OPTIM_MAX_SEGS 65535

/* One parameter tensor (72 bytes, a DEVICE array of them is the table).  Every pointer is a device pointer to n contiguous fp32,
 * 16-byte aligned; n >= 1, any tail of 1 - 3 elements behind the last whole quad is handled.  The last quad of g, p, m, v and ema
 * is READ whole (16 bytes from a 16-byte aligned address never leave the page of their first byte); nothing past element n - 1 is
 * used or written. */
typedef struct ditto_optim_seg {
    float* p;
    const float* g;
    float* m;                 /* exp_avg */
    float* v;                 /* exp_avg_sq */
    float* ema;               /* NULL: no average is kept for this tensor */
    uint64_t n;               /* elements */
    uint32_t slot0;           /* chunks of the segments in front of this one (its first partial slot) */
    uint32_t reserved;        /* 0 */
    double lr;                /* this tensor's learning rate ... */
    double weight_decay;      /* ... and decoupled weight decay */
} ditto_optim_seg;

/* The hyper-parameters every segment shares (HOST struct, read during the call). */
typedef struct ditto_optim_hyper {
    double beta1, beta2;      /* in [0, 1) */
    double eps;               /* >= 0 */
    double max_norm;          /* > 0: clip the global gradient norm to it; <= 0: off */
    double ema_decay;         /* in [0, 1]; used where a segment has an ema */
    int32_t skip_nonfinite;   /* 0 / 1 */
    int32_t reserved;         /* 0 */
} ditto_optim_hyper;

/* The DEVICE state block (128 bytes, 16-byte aligned, owned by the caller).  A fresh optimizer: beta1_pow = beta2_pow = 1.0 in both
 * slots, everything else 0 (clip is written before it is read).  The running state stands in two slots so that the one-launch step
 * can read it in every workgroup while one lane writes its successor: a step of phase f reads slot[f & 1] and writes
 * slot[(f + 1) & 1]; the caller passes f = 0, 1, 2, ... (its count of ditto_optim_adamw_step calls on this block, skipped steps
 * included).  A skipped step copies the slot with `skipped` + 1.  The report is written by the norm launches (and clip = 1, skip = 0
 * by a step without them). */
typedef struct ditto_optim_slot {
    double beta1_pow, beta2_pow;   /* beta^step, a running fp64 product */
    int64_t step;                  /* steps applied */
    int64_t skipped;               /* steps skipped */
} ditto_optim_slot;
typedef struct ditto_optim_state {
    ditto_optim_slot slot[2];      /* bytes 0 .. 63 */
    double norm;                   /* byte 64: the last pre-clip global norm */
    float norm32;                  /* byte 72: the same, rounded to fp32 */
    float clip;                    /* byte 76: the last clip factor */
    int32_t skip;                  /* byte 80: 1 if the last step was skipped */
    int32_t reserved[11];
} ditto_optim_state;

/* Bytes of the scratch (one fp64 partial per chunk, 256-byte aligned) of a table of n_chunks chunks; 0 with ditto_last_error set if
 * n_chunks is 0 or above 2^31 - 1. */
size_t ditto_optim_scratch_bytes(size_t n_chunks);

/* The two norm launches alone: state->norm, norm32, clip and skip as the step would decide them; no slot changes.  grid_limit > 0
 * caps the workgroups of the partial launch (0: the default) — the result's bits do not depend on it. */
int ditto_optim_grad_norm(const ditto_optim_seg* table, int n_seg, size_t n_chunks, const ditto_optim_hyper* hyper,
                          ditto_optim_state* state, void* scratch, size_t scratch_bytes, int grid_limit, ditto_stream_t stream);

/* One optimizer step of phase `phase` (see ditto_optim_state).  With max_norm <= 0 and skip_nonfinite == 0 this is ONE launch and
 * scratch may be NULL; otherwise norm partial, norm finish, apply.  Refused before any launch, with ditto_last_error set: null table /
 * hyper / state (DITTO_ERR_ARG), n_seg outside 1 .. DITTO_OPTIM_MAX_SEGS, n_chunks outside n_seg .. 2^31 - 1, phase < 0, grid_limit < 0,
 * a non-finite or out-of-range hyper-parameter, a misaligned state or scratch (DITTO_ERR_ARG), a scratch smaller than
 * ditto_optim_scratch_bytes(n_chunks) (DITTO_ERR_SIZE). */
int ditto_optim_adamw_step(const ditto_optim_seg* table, int n_seg, size_t n_chunks, const ditto_optim_hyper* hyper,
                           ditto_optim_state* state, int phase, void* scratch, size_t scratch_bytes, int grid_limit,
                           ditto_stream_t stream);

/* Exchange p and ema bit for bit in every segment that has an ema (one launch): sample from the averaged weights, and come back. */
int ditto_optim_swap(const ditto_optim_seg* table, int n_seg, size_t n_chunks, int grid_limit, ditto_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
