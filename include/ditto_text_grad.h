/* ditto_text_grad.h — C-ABI of the text side of training for classifier-free guidance (csrc/text_grad.hip, csrc/ditto_train.hip):
 * the gradient of a packed training step with respect to its text rows, and condition dropout — the selection of every utterance's
 * text between its own rows and a (learned) null embedding, forward and backward.
 *
 * A header of its own, beside include/ditto_hip.h and under its conventions (status codes, ditto_last_error, device pointers owned by
 * the caller, no allocation, no synchronisation, stream-ordered enqueues); DITTO_ABI_VERSION does not change with it and no struct
 * of ditto_hip.h grows.  As in ditto_train_rows.h, the two select entries take behind every pointer the BYTE SIZE of the buffer
 * that stands there and refuse — before any HIP call, with ditto_last_error naming the entry — what the kernel cannot serve:
 * DITTO_ERR_SHAPE (a dimension or a table entry outside what is stated below), then DITTO_ERR_ARG (a null or misaligned pointer), then
 * DITTO_ERR_SIZE (a buffer smaller than the extent the launch reads or writes there).
 */
#ifndef DITTO_TEXT_GRAD_H
#define DITTO_TEXT_GRAD_H

#include "ditto_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- condition dropout over a packed batch: one launch each way ----
 * The layout table, int32 [3B + 2], built by the caller on the host (varlen.cond_dropout_layout):
 *     cu_out  [B + 1]   offsets of the utterances in text_eff [S_out, dt]
 *     cu_text [B + 1]   offsets of the utterances in text [S_T, dt]
 *     drop    [B]       0: utterance b keeps its own rows (its length in text_eff is its length in text)
 *                       1: it runs unconditionally — its rows in text_eff are the T0 rows of null [T0, dt]
 * `table_host` is that table in HOST memory: it is read and validated before anything is launched (both offset rows start at 0,
 * increase strictly and end at S_out / S_T; drop is 0 / 1; every utterance's length in text_eff is T0 when dropped and its own
 * otherwise).  `table` is the same table in DEVICE memory, which the kernel reads; it clamps every index it forms from it, so a
 * device copy that differs from the host's cannot address outside a buffer.
 *
 * forward:   text_eff[cu_out[b] + r] = drop[b] ? null[r] : text[cu_text[b] + r]           — bit copies, 16 bytes per lane
 * backward:  d_text[cu_text[b] + r]  = drop[b] ? 0 : d_text_eff[cu_out[b] + r]             — every row of d_text is written
 *            d_null[r]               = sum over the dropped b, in ascending b, of d_text_eff[cu_out[b] + r]
 *                                      (one fp32 accumulator per element starting at 0, no atomics: the same bits every time;
 *                                      all zeros when nobody is dropped)
 * All data fp32, contiguous, 16-byte aligned, read / written whole.  dt % 4 == 0, 4 <= dt <= 65536; 1 <= B <= 65535; T0 >= 1;
 * B <= S_T, B <= S_out; S_T * dt and S_out * dt below 2^40. */
int ditto_text_select_packed(const float* text, size_t text_bytes, const float* null_rows, size_t null_rows_bytes,
                             const int32_t* table, size_t table_bytes, const int32_t* table_host, size_t table_host_bytes,
                             float* text_eff, size_t text_eff_bytes, int B, int S_T, int S_out, int T0, int dt,
                             ditto_stream_t stream);
int ditto_text_select_packed_bwd(const float* d_text_eff, size_t d_text_eff_bytes, const int32_t* table, size_t table_bytes,
                                 const int32_t* table_host, size_t table_host_bytes, float* d_text, size_t d_text_bytes,
                                 float* d_null, size_t d_null_bytes, int B, int S_T, int S_out, int T0, int dt,
                                 ditto_stream_t stream);

/* ---- the packed backward with the text gradient ----
 * ditto_train_backward_packed_layers (ditto_hip.h: the same arguments, the same gradients in `grads`, bit for bit) which also leaves
 *     d_text fp32 [S_T, text_dim] = sum_l dkv_l Wkv_l  +  the AdaLN pool path
 * the gradient of the caller's loss with respect to the `text` rows the forward was given.  Per layer, right after its cross-attention
 * backward has written dkv bf16 [S_T, 2d]: one bf16 GEMM against the K|V rows of cross_in_proj_weight (the transpose of the forward's
 * K/V projection of bf16(text)), accumulated into d_text in fp32 in the order l = num_layers - 1 .. 0.  In the tail:
 * dpooled [B, text_dim] = silu'(pooled) * (dmod W_ada_text), and dpooled[b] / T_b is added to every text row of utterance b, last.
 * No atomics: the same call twice gives the same bits.
 * In pieces (layer_from / layer_to): the piece that starts at the top layer zeroes d_text, every piece accumulates its layers, the
 * piece that ends at layer 0 adds the pool term — the same bits as the single call, given the same d_text to every piece.
 * d_text: required here (without one, ditto_train_backward_packed_layers is the entry), 16-byte aligned, S_T * text_dim * 4 bytes.
 * workspace: ditto_train_workspace_bytes_packed_text bytes (the plain backward's and, behind them, one layer's transposed K|V weight
 * and dpooled). */
size_t ditto_train_workspace_bytes_packed_text(const ditto_config* cfg, int B, int S, int max_N, int S_T, int max_T);
int ditto_train_backward_packed_text_layers(ditto_model_t m, const ditto_weights* w, const float* grad_eps, const float* x,
                                            const int64_t* t, const int32_t* cu_speech, const int32_t* cu_text, int B, int S, int max_N,
                                            int S_T, int max_T, const float* rope_cos, const float* rope_sin, float dropout_p,
                                            uint64_t seed, const void* tape, size_t tape_bytes, const ditto_grads* grads,
                                            void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts,
                                            int layer_from, int layer_to, float* d_text, size_t d_text_bytes);

#ifdef __cplusplus
}
#endif
#endif
