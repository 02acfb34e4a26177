/* ditto_project.h — C-ABI of projected guidance for packed guided sampling (csrc/guided_project.hip, csrc/ditto_api.hip): Adaptive
 * Projected Guidance, Sadat, Hilliges & Weber 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion
 * Models", Algorithm 1.  The guidance direction is taken in x0 space, split into the part parallel to the conditional x0 prediction
 * and the part orthogonal to it; the parallel part — what over-drives amplitude at a strong scale — is down-weighted by eta; the
 * direction may be capped in size (r) and carry a negative momentum (beta) across steps.
 *
 * A header of its own, beside include/ditto_hip.h and under its conventions (status codes, ditto_last_error, device pointers owned by
 * the caller, no allocation, no synchronisation, stream-ordered enqueues); DITTO_ABI_VERSION does not change with it and no struct
 * of ditto_hip.h grows.  The reference has no guided sampler: this is pinned by its own formulas, below.  What it does to the speech
 * of a trained model is not measured by anything in this library.
 *
 * ---- The arithmetic (the contract; tests/project_ref.py restates it in fp64 and as fp32 chains) ----
 * Per utterance b, over its generated window — window_span's rows [cu[b] + P_b, cu[b+1] - Q_b): prompt rows in front and suffix rows
 * behind are excluded — and all d columns; n = the window's element count.  All row data fp32:
 *   x     the conditional half of x2 [2S, d]             c, u   the two halves of eps2 [2S, d] (the network's outputs)
 *   m     the direction buffer `dir`, fp32 [S, d], in x0 space, row-aligned with the conditional half
 * and proj[b] = (kx, ke, w, eta, r, beta, use_prev).  kx and ke map a network output to the x0 prediction, D = kx x + ke out: the
 * kx / ke of the multistep schedule at the utterance's timestep (eps: 1 / alpha, -sigma / alpha; v: alpha, -sigma), so one kernel
 * serves both parameterisations.
 * Launch 1, direction and statistics, per element:
 *   dd = ke * (c - u)
 *   m' = use_prev ? fmaf(beta, m, dd) : dd            m' is stored; with use_prev == 0, m is never read (an utterance's first guided
 *                                                     step meets uninitialised memory)
 *   D  = fmaf(kx, x, ke * c)
 *   S_mm += m'^2, S_mD += m' D, S_DD += D^2           in fp64 (each product of the two fp32 values is exact in fp64; fma)
 *   The sums are cut exactly as the guidance rescale's: partials of DITTO_RESCALE_CHUNK_QUADS (4096) 16-byte quads of the utterance's
 *   own window — lane l of 256 adds quads l, l + 256, ... of the chunk, elements 0..3 in order; the 64 lanes of a wave meet in a fixed
 *   xor butterfly (32, 16, .., 1), the 4 waves in index order — combined per utterance by one wave: lane l adds partials l, l + 64, ...
 *   in order, then the same butterfly.  No atomics: the order depends on the utterance's chunk count only.
 * Finish, one wave per utterance, fp64, no contraction:
 *   rms   = sqrt(S_mm / n)
 *   rho   = r / rms  when r > 0 and rms is a finite number above r; otherwise 1
 *   p     = S_mD / S_DD  when S_DD is finite and positive; otherwise 0
 *   kappa = (w - 1) rho (1 - eta) p                    eta clamped into [0, 1] (NaN: 0) on the device
 *   fx = (float)(-kappa kx / ke), fc = (float)(1 - kappa), fd = (float)((w - 1) rho / ke);   ke == 0: (0, 1, 0)
 *   The stored m' is the value BEFORE thresholding, as in the paper's momentum buffer.
 * Launch 2, the update, per element:
 *   e = fmaf(fx, x, fmaf(fc, c, fd * m'))
 *   then the solver line of the plain entries, unchanged: x' = fmaf(a, x, fmaf(ce, e, cz z)) (strided; noise and Philox indexing as
 *   ditto_guided_update_packed_window / _tags_window) or the 2M lines of ditto_multistep_update_window; x' is written to both halves
 *   of x2.  u is not read in this launch.
 * In exact arithmetic kx x + ke e = D_c + (w - 1)(Delta_orth + eta Delta_par) with Delta = rho m' and D_c = kx x + ke c: the paper's
 * Algorithm 1.  eta = 1, r off, beta = 0 is plain classifier-free guidance, e = u + w (c - u).
 * DEVIATION from the paper: the threshold is on the direction's RMS over the window, sqrt(S_mm / n), not on its whole-sample norm
 * sqrt(S_mm): a norm over G_b d elements would make r depend on the utterance's length.
 *
 * An utterance's (fx, fc, fd), its m' and its x' are functions of its own window and parameters: not of its position, its neighbours,
 * B, S, max_N or the grid.  Context rows of x2, eps2 and dir are neither read nor written.  Bad offsets or lengths are clamped as in
 * the window entries (r0 into [0, S - 1], n_b into [1, S - r0], P_b into [0, n_b - 1], Q_b into [0, n_b - 1 - P_b]): wrong rows, never
 * an access outside the buffers.
 * Traffic per generated element: launch 1 reads x, c, u (and m with use_prev) and writes m', 16 - 20 B; launch 2 reads x, c, m' and
 * writes both halves, 20 B (+ 4 B noise buffer; + 8 B multistep history).
 * The same over a request stream's mixed layout, where only some utterances of a step are projected: include/ditto_project_stream.h.
 */
#ifndef DITTO_PROJECT_H
#define DITTO_PROJECT_H

#include "ditto_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one utterance's parameters of a projected-guidance step: a DEVICE array [B], 32 bytes each, 16-byte aligned */
typedef struct ditto_project_coef {
    float kx, ke;          /* x0 = kx x + ke out at the utterance's timestep */
    float w;               /* guidance scale */
    float eta;             /* weight of the parallel part, clamped into [0, 1] on the device */
    float r;               /* RMS threshold of the direction; <= 0 (or NaN): off */
    float beta;            /* momentum; read only with use_prev */
    int32_t use_prev;      /* 0: dir is written and never read */
    int32_t reserved;
} ditto_project_coef;

/* The scratch of one projected step: [coefs out | partials], each part 256-byte aligned — pcoef fp32 [B, 4] = (fx, fc, fd, 0) at byte
 * 0, then double [B, slots, 4] = (S_mm, S_mD, S_DD, 0) per chunk, slots = ceil(max_N d / 4 / 4096).  Returns 0 (and sets
 * ditto_last_error) unless B, max_N > 0 and d % 64 == 0. */
size_t ditto_guidance_project_bytes(int B, int max_N, int d);

/* ditto_guidance_project_packed: launch 1 and the finish alone.  x2, eps2 fp32 [2S, d]; dir fp32 [S, d], updated in place on the
 *   window rows; proj device ditto_project_coef [B]; cu device int32 [B + 1]; prompt_len, suffix_len NULL or device int32 [B]; scratch
 *   256-byte aligned, scratch_bytes >= ditto_guidance_project_bytes(B, max_N, d).  Afterwards the scratch opens with pcoef.
 *   DITTO_ERR_ARG: a null x2 / eps2 / dir / proj / cu / scratch, proj not 16-byte or scratch not 256-byte aligned; DITTO_ERR_SHAPE:
 *   d % 64 != 0 or the packed-batch conditions (B, S, max_N positive, max_N <= S, B <= S, B <= 65535); DITTO_ERR_SIZE: the scratch. */
int ditto_guidance_project_packed(const float* x2, const float* eps2, float* dir, const ditto_project_coef* proj, const int32_t* cu,
                                  const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, void* scratch,
                                  size_t scratch_bytes, ditto_stream_t stream);

/* ditto_guided_update_packed_project: launch 2 with the strided (DDIM) line.  pcoef: device fp32 [B, 4], 16-byte aligned (the head of
 *   the scratch); dir is only read; eps2's unconditional half is not read.  tags NULL: every utterance draws at the scalar `step`
 *   (ditto_guided_update_packed_window's noise); tags device uint32 [B]: utterance b at tags[b], no draw where cz[b] == 0
 *   (ditto_guided_update_packed_tags_window's).  noise packed fp32 [S, d] and seeds are exclusive; a, ce, cz fp32 [B]. */
int ditto_guided_update_packed_project(float* x2, const float* eps2, const float* dir, const float* pcoef, const float* noise,
                                       const int64_t* seeds, uint32_t step, const uint32_t* tags, const float* a, const float* ce,
                                       const float* cz, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                       int S, int max_N, int d, ditto_stream_t stream);
/* ditto_multistep_update_packed_project: launch 2 with the 2M lines of ditto_multistep_update_window on the history q fp32 [S, d]:
 *   exactly one of `step` (host: every utterance at that step) and `coefs` (device [B], 16-byte aligned); their w is not used. */
int ditto_multistep_update_packed_project(float* x2, const float* eps2, float* q, const float* dir, const float* pcoef,
                                          const ditto_multistep_coef* step, const ditto_multistep_coef* coefs, const int32_t* cu,
                                          const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d,
                                          ditto_stream_t stream);

/* The steps: ditto_guided_step_packed_window_opts' forward — one packed forward over [x; x] x [text; null], cu_speech [2B + 1], t
 *   [2B] — then launch 1 and the finish on its output, then the update above reading pcoef from the scratch.  Every argument is
 *   checked before any launch.  Workspace: ditto_packed_workspace_bytes(cfg, 2B, 2S, S_T). */
int ditto_guided_step_packed_project_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                          const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len, float* dir,
                                          const ditto_project_coef* proj, const float* noise, const int64_t* seeds, uint32_t step,
                                          const uint32_t* tags, const float* a, const float* ce, const float* cz, int B, int S, int max_N,
                                          int S_T, int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                          size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                          const ditto_call_opts* opts);
int ditto_guided_step_packed_multistep_project_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                    const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len,
                                                    const int32_t* suffix_len, float* q, float* dir, const ditto_project_coef* proj,
                                                    const ditto_multistep_coef* step, const ditto_multistep_coef* coefs, int B, int S,
                                                    int max_N, int S_T, int max_T, const float* rope_cos, const float* rope_sin,
                                                    void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                                                    ditto_stream_t stream, const ditto_call_opts* opts);

#ifdef __cplusplus
}
#endif
#endif
