/* ditto_refresh.h — C-ABI of guidance reuse in a request stream (csrc/guided_refresh.hip, csrc/ditto_api.hip): the fused update, and
 * the step around it, of a packed batch whose utterances each follow their own refresh schedule.  It continues the "Guidance reuse"
 * block of include/ditto_hip.h, which describes the approximation and its closed-batch entries.
 *
 * A header of its own, beside include/ditto_hip.h and under its conventions (status codes, ditto_last_error, device pointers owned by
 * the caller, no allocation, no synchronisation, stream-ordered enqueues); DITTO_ABI_VERSION does not change with it and no struct
 * of ditto_hip.h grows.
 */
#ifndef DITTO_REFRESH_H
#define DITTO_REFRESH_H

#include "ditto_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Guidance reuse over a request stream: every utterance stands at its own step of its own refresh schedule, so one step holds
 * utterances that refresh the direction (they need the unconditional forward), utterances that reuse the kept one and utterances that
 * are not guided at all.  What the approximation does to the speech of a trained model is not measured by anything in this library.
 * Layout: that of ditto_guided_update_packed_mixed with G = the REFRESHING utterances — x2, eps2 fp32 [S + S_G, d], every utterance
 *   in rows [0, S), the refreshing ones' unconditional copies compacted behind them in rows [S, S + S_G) in batch order; cu device
 *   int32 [B + G + 1] = [cu; S + cu_G[1:]]; partner device int32 [B]: the copy of utterance b in [0, G), or -1.
 * kind: device int32 [B], REQUIRED — 0 plain, 1 refresh, 2 reuse.  A value outside 0..2 counts as 0, and so does a 1 without a usable
 *   partner (partner[b] < 0 after its clamp, or n_b > S_G).
 * delta: fp32 [S, d], row-aligned with rows [0, S) of x2, REQUIRED: the kept direction of every utterance, on its generated rows.
 * ditto_guided_update_packed_refresh: per generated element of utterance b (rows [cu[b] + P_b, cu[b+1]))
 *   refresh  dl = c - u, e = fmaf(w[b], dl, u), u read at the copy's rows; x' goes to b's rows and to the copy's — the bits
 *            ditto_guided_update_packed_mixed writes for an utterance with a partner — and delta = dl on b's generated rows.
 *   reuse    e = fmaf(w[b] - 1.0f, delta, c) — ditto_guided_update_packed_reuse's LOAD line; x' goes to b's rows only; delta is read
 *            and never written.  With w[b] == 1, e == c exactly.
 *   plain    e = c — ditto_guided_update_packed_mixed without a partner; delta is neither read nor written.
 *   then x' = fmaf(a[b], x, fmaf(ce[b], e, cz[b] z)) with the per-utterance tags' noise: z = 0 (no Philox draw) where cz[b] == 0, so
 *   against a scalar-tag entry the bits agree where cz[b] != 0 (or without seeds).  For reuse and plain nothing in rows [S, S + S_G)
 *   is read or written.  Prompt rows of x2, eps2, delta and `noise` are neither read nor written.
 *   w, a, ce, cz, tags, seeds: [B]; noise packed fp32 [S, d]; prompt_len NULL or device int32 [B].  The conditions and clamps are
 *   ditto_guided_update_packed_mixed's (d % 64 == 0, 0 <= G <= B, G <= S_G <= S, S_G == 0 exactly when G == 0; partner[b] into
 *   [-1, G - 1], the copy's first row into [S, S + S_G - n_b], P_b into [0, n_b - 1]): a bad table gives wrong rows, never an access
 *   outside x2 [S + S_G, d] or delta [S, d].  A null delta or kind is DITTO_ERR_ARG; everything is checked before any launch.
 *   Traffic per generated element: refresh 24 B (x, c, u read; x', the copy and delta written), reuse 16 B, plain 12 B; + 4 B each
 *   with a noise buffer.
 * ditto_guided_step_packed_refresh_opts: ditto_guided_step_packed_mixed_opts' forward — one packed forward over the B + G utterances
 *   of x2, cond over [text_0 .. text_{B-1}; null_g ..] with cu_text [B + G + 1], t int64 [B + G] with a copy's t its partner's — then
 *   that update on its output.  G == 0: the forward over the B utterances alone (nobody refreshes); G == B: everyone does.
 *   Workspace: ditto_packed_workspace_bytes(cfg, B + G, S + S_G, S_T).
 * Not measured: the kernel alone has no timing of its own — it is HBM-bound like the updates it merges, and the stream's step is
 *   measured as a whole (tools/bench_stream_refresh.py). */
int ditto_guided_update_packed_refresh(float* x2, const float* eps2, float* delta, const float* noise, const int64_t* seeds,
                                       const uint32_t* tags, const float* w, const float* a, const float* ce, const float* cz,
                                       const int32_t* cu, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len, int B,
                                       int G, int S, int S_G, int max_N, int d, ditto_stream_t stream);
int ditto_guided_step_packed_refresh_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                          const int32_t* cu_text, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len,
                                          float* delta, const float* noise, const int64_t* seeds, const uint32_t* tags, const float* w,
                                          const float* a, const float* ce, const float* cz, int B, int G, int S, int S_G, int max_N,
                                          int S_T, int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                          size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);

#ifdef __cplusplus
}
#endif
#endif
