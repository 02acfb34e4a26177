/* ditto_project_stream.h — C-ABI of projected guidance (APG) in a request stream (csrc/guided_project_mixed.hip, csrc/ditto_api.hip):
 * the direction and statistics, the fused update and the step around them, of a packed batch whose utterances each stand at their
 * own step of their own schedule.  It continues include/ditto_project.h, which states the arithmetic and its closed-batch entries.
 *
 * A header of its own, beside include/ditto_hip.h and under its conventions (status codes, ditto_last_error, device pointers owned by
 * the caller, no allocation, no synchronisation, stream-ordered enqueues); DITTO_ABI_VERSION does not change with it and no struct
 * of ditto_hip.h or ditto_project.h grows.  What projected guidance does to the speech of a trained model is not measured by anything
 * in this library.
 *
 * Layout: that of ditto_guided_update_packed_mixed — x2, eps2 fp32 [S + S_G, d], every utterance in rows [0, S), the G utterances
 *   guided at this step (projected or not) with their unconditional copies compacted behind them in rows [S, S + S_G) in batch order;
 *   cu device int32 [B + G + 1] = [cu; S + cu_G[1:]]; partner device int32 [B]: the copy of utterance b in [0, G), or -1.  Conditions
 *   and clamps are that entry's (0 <= G <= B, G <= S_G <= S, S_G == 0 exactly when G == 0; partner[b] into [-1, G - 1], the copy's
 *   first row into [S, S + S_G - n_b], no copy when n_b > S_G, P_b into [0, n_b - 1]) plus d % 64 == 0.
 * dir: fp32 [S, d], row-aligned with rows [0, S) of x2: the x0-space direction m of every projected utterance, on its generated rows.
 * kind: device int32 [B], REQUIRED — 0 plain, 1 guided without projection, 3 projected.  2 is left unused (it is the reuse kind of
 *   include/ditto_refresh.h); every value outside {1, 3} counts as 0, and so does a 1 or a 3 without a usable partner (partner[b] < 0
 *   after its clamp, or n_b > S_G).
 * proj: device ditto_project_coef [B], 16-byte aligned; read for kind 3 only.
 * scratch: ditto_guidance_project_bytes(B, max_N, d) with the layout it has in include/ditto_project.h: pcoef fp32 [B, 4] at byte 0,
 *   then the fp64 partials; 256-byte aligned.
 * A bad cu, partner, kind or prompt_len gives wrong rows, never an access outside x2, eps2 [S + S_G, d], dir [S, d] or the scratch.
 * Prompt rows of x2, eps2, dir and `noise` are neither read nor written.
 *
 * HBM traffic per generated element, by kind:
 *   projected   launch 1 reads x, c, u (and m with use_prev) and writes m': 16 - 20 B; launch 2 reads x, c, m' and writes x' and the
 *               copy: 20 B
 *   guided      launch 1 nothing; launch 2 reads x, c, u and writes x' and the copy: 20 B
 *   plain       launch 1 nothing; launch 2 reads x, c and writes x': 12 B
 *   + 4 B in launch 2 with a noise buffer; 0 B per prompt element.  The finish reads 32 B per chunk of 4096 quads and writes 16 B per
 *   utterance.
 */
#ifndef DITTO_PROJECT_STREAM_H
#define DITTO_PROJECT_STREAM_H

#include "ditto_project.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ditto_guidance_project_packed_mixed: launch 1 and the finish.  For a kind-3 utterance exactly ditto_guidance_project_packed's
 *   arithmetic — the chunk cut, the lane order, the butterfly, the fp64 finish, use_prev — with u read at the copy's rows instead of
 *   S rows further down: pcoef[b] and m' have the closed entry's bits for the same window and parameters.  Workgroups of the other
 *   kinds leave on a uniform branch: they read nothing of x2, eps2 or dir, write nothing to dir, and get pcoef[b] = (0, 1, 0, 0).
 *   DITTO_ERR_ARG: a null x2 / eps2 / dir / proj / cu / partner / kind / scratch, x2 / eps2 / dir / proj not 16-byte or the scratch not
 *   256-byte aligned; DITTO_ERR_SHAPE: d % 64 != 0, the packed-batch conditions or the layout's; DITTO_ERR_SIZE: the scratch. */
int ditto_guidance_project_packed_mixed(const float* x2, const float* eps2, float* dir, const ditto_project_coef* proj,
                                        const int32_t* cu, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len, int B,
                                        int G, int S, int S_G, int max_N, int d, void* scratch, size_t scratch_bytes,
                                        ditto_stream_t stream);

/* ditto_guided_update_packed_project_mixed: launch 2.  Per generated element of utterance b (rows [cu[b] + P_b, cu[b+1])):
 *   projected  e = fmaf(fx, x, fmaf(fc, c, fd m')) with (fx, fc, fd) = pcoef[b]; x' goes to b's rows and to the copy's; u is not read
 *              — ditto_guided_update_packed_project's bits (tags form).
 *   guided     e = fmaf(w[b], c - u, u); x' goes to both — ditto_guided_update_packed_mixed's bits for an utterance with a partner.
 *   plain      e = c; x' goes to b's rows only — that entry's bits without a partner.
 *   then x' = fmaf(a[b], x, fmaf(ce[b], e, cz[b] z)) with the per-utterance tags' noise: no Philox draw where cz[b] == 0.  dir is only
 *   read, and for kind 3 only.  pcoef: device fp32 [B, 4], 16-byte aligned (the head of the scratch).  noise packed fp32 [S, d],
 *   16-byte aligned, and seeds are exclusive; seeds need tags (uint32 [B]); w, a, ce, cz fp32 [B]. */
int ditto_guided_update_packed_project_mixed(float* x2, const float* eps2, const float* dir, const float* pcoef, const float* noise,
                                             const int64_t* seeds, const uint32_t* tags, const float* w, const float* a, const float* ce,
                                             const float* cz, const int32_t* cu, const int32_t* partner, const int32_t* kind,
                                             const int32_t* prompt_len, int B, int G, int S, int S_G, int max_N, int d,
                                             ditto_stream_t stream);

/* ditto_guided_step_packed_project_mixed_opts: ditto_guided_step_packed_mixed_opts' forward — one packed forward over the B + G
 *   utterances of x2, cond over [text_0 .. text_{B-1}; null_g ..] with cu_text [B + G + 1], t int64 [B + G] with a copy's t its
 *   partner's — then the two entries above on its output, the update reading pcoef from the scratch.  Every argument is checked before
 *   any launch.  Workspace: ditto_packed_workspace_bytes(cfg, B + G, S + S_G, S_T). */
int ditto_guided_step_packed_project_mixed_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                                const int32_t* cu_text, const int32_t* partner, const int32_t* kind,
                                                const int32_t* prompt_len, float* dir, const ditto_project_coef* proj, const float* noise,
                                                const int64_t* seeds, const uint32_t* tags, const float* w, const float* a,
                                                const float* ce, const float* cz, int B, int G, int S, int S_G, int max_N, int S_T,
                                                int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                                size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                                const ditto_call_opts* opts);

#ifdef __cplusplus
}
#endif
#endif
