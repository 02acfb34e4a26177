/* ditto_hip.h — C-ABI of libditto_hip.so: the MI355X (gfx950) DiT denoise path.
 *
 * The reference (Tikai7/DiTTO-TTS) is pure Python with no FFI or operator registry;
 * its boundary for this path is the nn.Module surface.  This header
 * is the *new* boundary underneath that surface: each entry point names the reference
 * Python function (file:line, relative to the reference repo) whose arithmetic it
 * replaces.  The Python binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types, no exceptions.
 *  - Every function returns a ditto_status (0 = ok) and never aborts;
 *    ditto_last_error() returns a thread-local message for the last failure.
 *  - All tensor pointers are DEVICE pointers owned by the caller.  The library
 *    allocates no device memory and never synchronises: one call = one
 *    stream-ordered enqueue on `stream` (a hipStream_t; NULL = the default stream),
 *    so a caller may capture any call into a hipGraph.
 *  - Row-major, contiguous.  B = batch, N = latent length, T = text length,
 *    d = hidden_dim, H = num_heads, dh = d / H, L = num_layers, M = B*N.
 *  - fp32 in / fp32 out at the model boundary (what the reference's callers hold);
 *    bf16 operands with fp32 accumulation inside (MFMA).
 */
#ifndef DITTO_HIP_H
#define DITTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DITTO_ABI_VERSION 10

typedef enum ditto_status {
    DITTO_OK = 0,
    DITTO_ERR_ARG = 1,        /* null pointer / bad enum */
    DITTO_ERR_SHAPE = 2,      /* unsupported shape (message says which constraint) */
    DITTO_ERR_HIP = 3,        /* a HIP runtime call failed */
    DITTO_ERR_SIZE = 4        /* caller-provided arena / workspace / cond buffer too small */
} ditto_status;

typedef void* ditto_stream_t;            /* hipStream_t */
typedef struct ditto_model* ditto_model_t;

/* Per-call options (ABI 9).  Four switches decide WHICH BITS an utterance gets — the kernel class its launch takes, the type of
 * the residual stream, the fused full-row launches, the fused norm2 + q-projection — so they belong to a CALL, not to the
 * process: the *_opts entry points take them as an argument, and ditto_call_opts_push / _pop put them in force for every call
 * the CALLING THREAD makes in between.  Each field: -1 = inherit (the thread's enclosing push scope, else the process default of
 * ditto_set_option).  A call runs entirely on its calling thread (it only enqueues), so threads with different options do not
 * interfere; handles stay immutable.
 *   class_rows    > 0: decide the kernel class as a batch of that many rows (B * N of the UNSPLIT batch) would — what a caller
 *                 that splits one batch over launches or GPUs passes so that sharding changes no bit ("fr_class_rows");
 *                 0: the launch's own rows.
 *   residual_bf16 0 / 1 ("residual_bf16").      fr_mask 0 .. 3 ("fr_mask").      lnq 0 / 16 / 32 ("lnq").
 *   reserved      must be zero. */
typedef struct ditto_call_opts {
    int32_t class_rows;
    int32_t residual_bf16;
    int32_t fr_mask;
    int32_t lnq;
    int32_t reserved[4];
} ditto_call_opts;

/* DiTTO.__init__ keyword arguments, reference src/model/DiTTO.py:10-19.
 * Shapes: hidden_dim % 64 == 0 and <= 2048; hidden_dim % num_heads == 0 with an EVEN head_dim (half-split RoPE).  head_dim 64
 * runs the fused attention kernels; any other multiple of 64 (e.g. the shipped 1-head / 768 config) the GEMM-composed attention;
 * head_dim % 64 != 0 (the reference takes it: src/components/DiT.py:78-86; e.g. 1152 / 16 = 72) runs forward-only on heads
 * PADDED to the next multiple of 64 inside the block — zero weight rows / columns, so no result changes; the arena, cond and
 * workspace sizes grow accordingly (always take them from the *_bytes queries); training and fp8 linears refuse such shapes. */
typedef struct ditto_config {
    int32_t hidden_dim;        /* d        (768)  */
    int32_t num_layers;        /* L        (12)   */
    int32_t num_heads;         /* H        (12)   */
    int32_t time_dim;          /*          (256)  */
    int32_t text_dim;          /* must equal hidden_dim: reference src/components/DiT.py:90-91 */
    int32_t diffusion_steps;   /* rows of t_embedding (1000; 50 for the benchmark loop) */
    int32_t flags;             /* DITTO_CFG_* */
} ditto_config;

/* QKV, fc1|gate and fc2 GEMMs with OCP fp8 (e4m3) operands on the MX-scaled MFMA (BASELINE config 5): weights
 * quantised per output row at ditto_model_create, activations by the producing LayerNorm / gated-MLP epilogue;
 * fp32 accumulation, bf16 attention, fp32 residual stream unchanged.  Needs hidden_dim % 128 == 0. */
#define DITTO_CFG_FP8_LINEAR 1

/* fp32 device pointers, named after the reference state_dict keys.
 * `blocks.i.attn.out_proj.*` and `blocks.i.rotary.inv_freq` are intentionally absent:
 * the reference never reads them on this path (src/components/DiT.py:134-139). */
typedef struct ditto_layer_weights {
    const float* norm1_weight;  const float* norm1_bias;                 /* blocks.i.norm1.*            [d]      */
    const float* attn_in_proj_weight;  const float* attn_in_proj_bias;   /* blocks.i.attn.in_proj_*     [3d,d],[3d] */
    const float* norm2_weight;  const float* norm2_bias;                 /* blocks.i.norm2.*                     */
    const float* cross_in_proj_weight; const float* cross_in_proj_bias;  /* blocks.i.cross_attn.in_proj_*        */
    const float* cross_out_proj_weight; const float* cross_out_proj_bias;/* blocks.i.cross_attn.out_proj.* [d,d],[d] */
    const float* norm3_weight;  const float* norm3_bias;                 /* blocks.i.norm3.*                     */
    const float* mlp_fc1_weight; const float* mlp_fc1_bias;              /* blocks.i.mlp_fc1.*          [4d,d],[4d] */
    const float* gate_weight;    const float* gate_bias;                 /* blocks.i.gate.*             [4d,d],[4d] */
    const float* mlp_fc2_weight; const float* mlp_fc2_bias;              /* blocks.i.mlp_fc2.*          [d,4d],[d]  */
} ditto_layer_weights;

typedef struct ditto_weights {
    const float* t_embedding_weight;                                     /* [steps, time_dim] */
    const float* time_embed_0_weight; const float* time_embed_0_bias;    /* [td,td],[td] */
    const float* time_embed_2_weight; const float* time_embed_2_bias;
    const float* ada_time_mlp_weight; const float* ada_time_mlp_bias;    /* ada_ln.time_mlp.1.* [2d,td],[2d] */
    const float* ada_text_mlp_weight; const float* ada_text_mlp_bias;    /* ada_ln.text_mlp.1.* [2d,dt],[2d] */
    const float* proj_in_weight;  const float* proj_in_bias;             /* [d,d],[d] */
    const float* proj_out_weight; const float* proj_out_bias;
    const float* rotary_inv_freq;                                        /* rotary.inv_freq [dh/2] */
    const ditto_layer_weights* layers;                                   /* HOST array [num_layers] */
} ditto_weights;

/* ---- library ---------------------------------------------------------------------- */
int         ditto_abi_version(void);
const char* ditto_last_error(void);

/* ---- sizes (host-only arithmetic, no GPU needed) ------------------------------------ */
/* bytes of device arena ditto_model_create packs the weights into */
size_t ditto_arena_bytes(const ditto_config* cfg);
/* bytes of the per-batch conditioning buffer: cached cross-attention K/V of every layer
 * [B*T, L*2d] bf16 + the text half of the AdaLN modulation [B, 2d] fp32 */
size_t ditto_cond_bytes(const ditto_config* cfg, int B, int T);
/* bytes of scratch ditto_forward / ditto_text_precompute need for (B, N, T) */
size_t ditto_workspace_bytes(const ditto_config* cfg, int B, int N, int T);

/* ---- model handle --------------------------------------------------------------------
 * Packs DiTTO's parameters (reference src/model/DiTTO.py:36-64, src/components/DiT.py:78-98)
 * for the kernels: bf16 weights, fused [W_fc1;W_gate] interleave, all layers' cross-attention
 * K/V projections concatenated, [W_proj_in | W_proj_out] concatenated along K, and the
 * timestep -> AdaLN (scale,shift) table  time_mlp(time_embed(t_embedding[t]))  for every t
 * (src/model/DiTTO.py:75-76 + src/components/DiT.py:30: depends on t and weights only).
 * The handle is immutable afterwards; concurrent calls on different streams are safe.
 * If EVERY model-level pointer of `w` (everything except `layers`) is NULL the handle is "blocks-only":
 * ditto_block_forward and ditto_text_precompute (K/V only) work, ditto_forward / ditto_rope_tables refuse. */
int ditto_model_create(const ditto_config* cfg, const ditto_weights* w, void* arena, size_t arena_bytes,
                       ditto_stream_t stream, ditto_model_t* out);
int ditto_model_destroy(ditto_model_t m);

/* RotaryEmbedding.forward (src/components/DiT.py:56-59): cos/sin of n*inv_freq[j],
 * cos_out/sin_out fp32 [N, dh/2] */
int ditto_rope_tables(ditto_model_t m, int N, float* cos_out, float* sin_out, ditto_stream_t stream);

/* Step-invariant text work, once per batch of utterances (the reference redoes it every step,
 * SURVEY.md App. B-9): the text half of GlobalAdaLN (src/components/DiT.py:27,31: mean-pool over T,
 * SiLU, Linear) and every layer's cross-attention K/V in-projection of text_emb
 * (src/components/DiT.py:144-148 -> torch F.multi_head_attention_forward packed in-projection).
 * text fp32 [B,T,text_dim] -> cond (ditto_cond_bytes). */
int ditto_text_precompute(ditto_model_t m, const float* text, int B, int T, void* cond, size_t cond_bytes,
                          void* workspace, size_t workspace_bytes, ditto_stream_t stream);

/* DiTTO.forward(x, text_emb, t)  (src/model/DiTTO.py:66-94) with text_emb given as `cond`.
 * x fp32 [B,N,d], t int64 [B] (device), rope_cos/sin from ditto_rope_tables(N), eps_out fp32 [B,N,d]. */
int ditto_forward(ditto_model_t m, const float* x, const void* cond, const int64_t* t, int B, int N, int T,
                  const float* rope_cos, const float* rope_sin, float* eps_out,
                  void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* the same call with its options as an argument (opts == NULL: every field inherits) */
int ditto_forward_opts(ditto_model_t m, const float* x, const void* cond, const int64_t* t, int B, int N, int T,
                       const float* rope_cos, const float* rope_sin, float* eps_out,
                       void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
/* Variable-length batches (padded layout): utterance b is x[b, :speech_len[b]] and text[b, :text_len[b]]; the rows past them are
 * padding, whose contents (NaN / Inf included) never reach a valid row.  speech_len / text_len: DEVICE int32 [B], non-NULL.
 * Precondition (not checked: that would need a sync): 1 <= speech_len[b] <= N, 1 <= text_len[b] <= T; the kernels clamp into that
 * range, so a bad value gives wrong rows but never an out-of-bounds access.  head_dim 64 only (DITTO_ERR_SHAPE otherwise).
 * ditto_text_precompute_varlen: the text mean-pool of GlobalAdaLN over the utterance's own T_b rows (the same association as
 * the dense kernel at T = T_b).  ditto_forward_varlen_opts: `cond` from ditto_text_precompute_varlen with the same text_len;
 * eps rows >= speech_len[b] are written 0 (one extra launch).  Every other launch is row-wise and also computes the padding rows. */
int ditto_text_precompute_varlen(ditto_model_t m, const float* text, const int32_t* text_len, int B, int T, void* cond,
                                 size_t cond_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream);
int ditto_forward_varlen_opts(ditto_model_t m, const float* x, const void* cond, const int64_t* t, const int32_t* speech_len,
                              const int32_t* text_len, int B, int N, int T, const float* rope_cos, const float* rope_sin,
                              float* eps_out, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                              const ditto_call_opts* opts);
/* Thread-scoped form for every other entry point (ditto_block_forward*, the unit-test kernels, a caller's own helper that
 * makes several calls): `opts` are in force for the calls THIS THREAD makes until the matching pop.  Nests (depth <= 16);
 * fields at -1 inherit the enclosing scope.  ditto_call_opts_pop without a push is an error. */
int ditto_call_opts_push(const ditto_call_opts* opts);
int ditto_call_opts_pop(void);
/* what a call made by this thread NOW, without an opts argument, would run under: every field resolved (scope, else process
 * default), none -1 */
int ditto_call_opts_current(ditto_call_opts* out);

/* One DiT block, DiT.forward(x, text_emb, time_emb, rotary_pos) (src/components/DiT.py:100-157), in place on the
 * fp32 residual stream h [B,N,d].  `layer` selects the packed weights, `cond_layer` the K/V slice of `cond`
 * (a standalone block uses a 1-layer handle and cond_layer = 0).  time_emb is not an input: the reference's
 * block ignores it. */
int ditto_block_forward(ditto_model_t m, int layer, float* h, const void* cond, int cond_layer, int B, int N, int T,
                        const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                        ditto_stream_t stream);
/* The same block with taps for segment-wise parity (src/components/DiT.py:139 and :148): `tap_self` / `tap_cross`
 * (fp32 [B,N,d], either may be NULL) receive the residual stream after the self-attention segment and after the
 * cross-attention segment; h ends as after the gated MLP (:155). */
int ditto_block_forward_taps(ditto_model_t m, int layer, float* h, const void* cond, int cond_layer, int B, int N,
                             int T, const float* rope_cos, const float* rope_sin, float* tap_self, float* tap_cross,
                             void* workspace, size_t workspace_bytes, ditto_stream_t stream);

/* GlobalAdaLN.forward(x, time_emb, text_emb) as a standalone module (src/components/DiT.py:25-40): explicit
 * time_emb fp32 [B,time_dim] instead of a timestep; weights are the module's own fp32 device tensors
 * (time_mlp.1.*, text_mlp.1.*).  out fp32 [B,N,d]. */
size_t ditto_global_adaln_scratch_bytes(int B, int d, int time_dim, int text_dim);
int ditto_global_adaln(const float* x, const float* time_emb, const float* text_emb, const float* time_w,
                       const float* time_b, const float* text_w, const float* text_b, int B, int N, int T, int d,
                       int time_dim, int text_dim, float* out, void* scratch, size_t scratch_bytes,
                       ditto_stream_t stream);

/* RotaryEmbedding.apply_rope(pos, t) (src/components/DiT.py:61-72): pos fp32 [N,dh] ANGLES (the tensor
 * RotaryEmbedding.forward returns), t fp32 [B,N,H,dh] -> out (not in place). */
int ditto_apply_rope_f32(const float* pos, const float* t, float* out, int B, int N, int H, int dh,
                         ditto_stream_t stream);

/* SpeechGenerator.__p_sample's update (src/model/SpeechGenerator.py:137-145), in place on x:
 *   x <- (x - (1-alpha_t)/sqrt(1-acp_t) * eps)/sqrt(alpha_t) + [t>0]*sqrt(beta_t)*noise
 * betas/alphas/alphas_cumprod fp32 [steps] (device), t int64 [B] (device), noise may be NULL only
 * if every t == 0 is guaranteed by the caller (it is then never read). */
int ditto_p_sample_update(float* x, const float* eps, const float* noise, const int64_t* t,
                          const float* betas, const float* alphas, const float* alphas_cumprod,
                          int B, size_t elems_per_utt, ditto_stream_t stream);

/* One reverse-diffusion step = ditto_forward + ditto_p_sample_update (SpeechGenerator.__p_sample,
 * src/model/SpeechGenerator.py:130-147); eps scratch lives in the workspace. */
int ditto_p_sample(ditto_model_t m, float* x, const void* cond, const int64_t* t, const float* noise,
                   const float* betas, const float* alphas, const float* alphas_cumprod,
                   int B, int N, int T, const float* rope_cos, const float* rope_sin,
                   void* workspace, size_t workspace_bytes, ditto_stream_t stream);
int ditto_p_sample_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const float* noise,
                        const float* betas, const float* alphas, const float* alphas_cumprod,
                        int B, int N, int T, const float* rope_cos, const float* rope_sin,
                        void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);

/* The sampling loop, SpeechGenerator.__sample_latents (src/model/SpeechGenerator.py:149-164), as ONE stream-ordered
 * enqueue: for t_val = t_begin, t_begin-1, ..., t_end:  x <- p_sample(x, full(B, t_val), cond).  `noise` holds the
 * N(0,1) draws of the steps in execution order, fp32 [t_begin - t_end + 1, B, N, d] (the caller's RNG: the library has
 * none; it may be NULL only when t_begin == t_end == 0).  t_scratch: int64 [B] device scratch the loop fills.
 * A caller that wants the whole loop in a hipGraph captures this single call. */
int ditto_denoise_steps(ditto_model_t m, float* x, const void* cond, int t_begin, int t_end, const float* noise,
                        const float* betas, const float* alphas, const float* alphas_cumprod, int B, int N, int T,
                        const float* rope_cos, const float* rope_sin, int64_t* t_scratch, void* workspace,
                        size_t workspace_bytes, ditto_stream_t stream);
int ditto_denoise_steps_opts(ditto_model_t m, float* x, const void* cond, int t_begin, int t_end, const float* noise,
                             const float* betas, const float* alphas, const float* alphas_cumprod, int B, int N, int T,
                             const float* rope_cos, const float* rope_sin, int64_t* t_scratch, void* workspace,
                             size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);

/* Per-utterance counter-based N(0,1) (no reference counterpart: the reference draws `torch.randn_like` from torch's
 * global generator, src/model/SpeechGenerator.py:141,154, a stream that cannot be sharded over GPUs).
 * out[b, i] = Philox4x32-10(key = seeds[b], counter = (i / 4, step, tag)) -> Box-Muller: a function of (seeds[b], step, i)
 * only, so an utterance's noise does not depend on its batch, its place in it or the GPU it runs on (SURVEY.md 8e:
 * per-utterance seeds make the sharded result independent of the world size).  seeds int64 [B] (device).
 * ditto_p_sample_seeded = ditto_p_sample with the step's noise generated inside the update kernel: bit-identical to
 * ditto_noise_normal(step) followed by ditto_p_sample(noise), without the noise buffer. */
int ditto_noise_normal(float* out, const int64_t* seeds, uint32_t step, int B, size_t elems_per_utt,
                       ditto_stream_t stream);
int ditto_p_sample_seeded(ditto_model_t m, float* x, const void* cond, const int64_t* t, const int64_t* seeds,
                          uint32_t step, const float* betas, const float* alphas, const float* alphas_cumprod, int B,
                          int N, int T, const float* rope_cos, const float* rope_sin, void* workspace,
                          size_t workspace_bytes, ditto_stream_t stream);
int ditto_p_sample_seeded_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const int64_t* seeds,
                               uint32_t step, const float* betas, const float* alphas, const float* alphas_cumprod, int B,
                               int N, int T, const float* rope_cos, const float* rope_sin, void* workspace,
                               size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
/* ditto_p_sample_opts over a variable-length batch (the sampler's noises= path): rows >= speech_len[b] of x are written 0 */
int ditto_p_sample_varlen_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const float* noise,
                               const int32_t* speech_len, const int32_t* text_len, const float* betas, const float* alphas,
                               const float* alphas_cumprod, int B, int N, int T, const float* rope_cos, const float* rope_sin,
                               void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
/* ditto_p_sample_seeded over a variable-length batch (lengths as ditto_forward_varlen_opts): the seeded update keeps the element
 * index of the padded layout (row-major within the utterance: the index it has at the utterance's own length), and rows
 * >= speech_len[b] of x are written 0 (one extra launch). */
int ditto_p_sample_seeded_varlen_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const int64_t* seeds,
                                      const int32_t* speech_len, const int32_t* text_len, uint32_t step, const float* betas,
                                      const float* alphas, const float* alphas_cumprod, int B, int N, int T, const float* rope_cos,
                                      const float* rope_sin, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                                      const ditto_call_opts* opts);

/* DiTTO.q_sample (src/model/DiTTO.py:106-126), bug-for-bug: `buffer` is the module's
 * `alphas_cumprod` buffer, which holds clipped betas.  out may alias x_start. */
int ditto_q_sample(const float* x_start, const float* noise, const int64_t* t, const float* buffer,
                   float* out, int B, size_t elems_per_utt, ditto_stream_t stream);

/* ---- single kernels, exported for unit parity tests ------------------------------------ */
/* nn.LayerNorm(d) eps=1e-5 (src/components/DiT.py:84,89,94,105,143,152): x fp32 [M,d] -> bf16 [M,d];
 * gamma/beta may both be NULL (elementwise_affine=False, src/components/DiT.py:23). */
int ditto_layernorm_bf16(const float* x, const float* gamma, const float* beta, void* out_bf16,
                         int M, int d, ditto_stream_t stream);

/* out[M,N] = A[M,K](bf16, row stride lda) * W[N,K]^T(bf16) + bias[N](fp32) — F.linear.
 * epilogue: 0 = bf16 out; 1 = fp32 out = acc + bias + residual (residual may alias out; may be NULL);
 *           4 = fp32 out = acc + bias;
 *           6 = bf16 out = relu(acc + bias)  (linear1 of nn.TransformerDecoderLayer, src/model/SpeechLP.py:23-28);
 *           3 = gated MLP (src/components/DiT.py:153-155): W/bias rows interleaved in blocks of 16
 *               [16 x mlp_fc1 | 16 x gate | ...], out bf16 [M, N/2] = gelu_erf(a) * sigmoid(g), ldo = N/2 or more. */
int ditto_gemm_bf16(const void* A, int lda, const void* W, const float* bias, const float* residual,
                    void* out, int ldo, int M, int N, int K, int epilogue, ditto_stream_t stream);

/* Every bf16 GEMM epilogue with every stride (tests/test_gpu_gemm_epilogues.py): the fields of a bf16 launch as the library's own
 * callers fill them.  epilogue (csrc/kernels.h GemmEpilogue): 0, 1, 3, 4, 6 as ditto_gemm_bf16;
 *   2 = QKV + RoPE: out bf16 [M, ldo]; columns < rope_cols get the half-split rotation (pairs (j, j + 32) of each 64-wide head,
 *       src/components/DiT.py:52-72) at position row % rope_rows_per_batch; angles from rope_freq_rev (fp32 [32] = inv_freq / (2 pi))
 *       if given, else from the tables rope_cos / rope_sin (fp32 [positions, 32]; both are required either way);
 *   9 = the same over a packed batch: the position of row r is rope_pos[r] (int32 [M]);
 *   8 = epilogue 3 that also writes the pre-activations acc + bias to out2_bf16 [M, ldo2] (packed column order), N % 256 == 0;
 *   7 = the gated MLP's backward on the fc2 dgrad: acc = dact [M, N]; pre_bf16 [M, ldpre] = the forward's pre-activations;
 *       out bf16 [M, 2 N] = [da | dg] in the packed order; colsum_partial fp32 [2 * ceil(M / 256), 2 N] = the column sums of the
 *       rounded output, one row per 128 rows.  No bias.  Only where the library itself fuses it (N % 256 == 0, N >= 2048, >= 144
 *       tiles of 256 x 256, "gemm_tile" 0 or 256): DITTO_ERR_SHAPE otherwise.
 *   5 (fp8 output) is ditto_gemm_fp8's: DITTO_ERR_ARG here.
 * ldw 0 = K; w_rows 0 = N (W rows >= w_rows are not read; the output columns they would give are unspecified); rows of `out`
 * start at multiples of 16 bytes.  Which tile structure runs is decided as for ditto_gemm_bf16 ("gemm_tile", "gemm_flags",
 * "pp_nb"); *structure_out (may be NULL) receives the one that ran, as the value "gemm_tile" would force (127 = the 128 x 128
 * kernel's deep-prefetch form), 0 if nothing was launched. */
typedef struct ditto_gemm_epilogue_args {
    const void* A; int lda;
    const void* W; int ldw; int w_rows;
    const float* bias;
    const float* residual; int ldr;
    void* out; int ldo;
    void* out2_bf16; int ldo2;
    const float* rope_cos; const float* rope_sin; int rope_rows_per_batch; int rope_cols;
    const float* rope_freq_rev;
    const int32_t* rope_pos;
    const void* pre_bf16; int ldpre;
    float* colsum_partial;
    int M, N, K;
} ditto_gemm_epilogue_args;
int ditto_gemm_epilogue_bf16(const ditto_gemm_epilogue_args* args, int epilogue, int* structure_out, ditto_stream_t stream);

/* softmax(q k^T * scale) v per (batch, head), no mask (src/components/DiT.py:131-134;
 * torch functional.py MHA math).  q/k/v/out bf16, element strides given per row; head h occupies
 * columns [h*dh, (h+1)*dh) of each row; rows of batch b start at b*Sq (q,out) / b*Skv (k,v). */
int ditto_attention_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                         void* out, int ldo, int B, int H, int Sq, int Skv, int dh, float scale,
                         void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* scratch bytes ditto_attention_bf16 needs: 0 at dh = 64 (the fused kernels), the chunked score / probability / V^T arrays of the
 * GEMM-composed path otherwise */
size_t ditto_attention_workspace_bytes(int B, int H, int Sq, int Skv, int dh);
/* the self-attention's residual epilogue (src/components/DiT.py:131-139: the head merge added to the stream, no out-projection):
 * resid_out[b*Sq+i, h*dh+c] = resid_in[b*Sq+i, h*dh+c] + (softmax(q k^T * scale) v)[...], rows of ldr elements, fp32 or (resid_is_bf16,
 * head_dim 64 only) bf16.  resid_in NULL or == resid_out: in place (the model's case).  q / k / v, scale, workspace and attn_flags
 * as ditto_attention_bf16; the same dispatch as the model's self-attention. */
int ditto_attention_resid_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid_in,
                               void* resid_out, int ldr, int resid_is_bf16, int B, int H, int Sq, int Skv, int dh, float scale,
                               void* workspace, size_t workspace_bytes, ditto_stream_t stream);

/* Variable-length batches (padded layout): utterance b owns query rows [b*Sq, b*Sq + q_len[b]) and key / value rows
 * [b*Skv, b*Skv + kv_len[b]); the rows past them are padding — never read (NaN / Inf there reach nothing) and never written.
 * q_len / kv_len: DEVICE int32 [B], either may be NULL (= the whole padded Sq / Skv), not both.  Precondition (the library cannot
 * read device memory without a sync): 1 <= q_len[b] <= Sq and 1 <= kv_len[b] <= Skv; the kernels clamp into that range, so a bad
 * value gives wrong rows but never an out-of-bounds access.  head_dim 64 only; q carries scale * log2(e) (the model's packed q:
 * attn_flags 16 of the dense entries is implied); row strides are multiples of 8 elements.  The dense entries' dispatch is not
 * used: every varlen launch runs attn64q (attn64p's exact body for an utterance of <= 64 keys; attn_flags 1048576: attn64p alone),
 * and an utterance's bits depend only on its own rows and lengths. */
int ditto_attention_varlen_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                                const int32_t* q_len, const int32_t* kv_len, int B, int H, int Sq, int Skv, int dh,
                                ditto_stream_t stream);
/* the residual form (as ditto_attention_resid_bf16): stream rows past q_len[b] are left untouched */
int ditto_attention_resid_varlen_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid_in,
                                      void* resid_out, int ldr, int resid_is_bf16, const int32_t* q_len, const int32_t* kv_len,
                                      int B, int H, int Sq, int Skv, int dh, ditto_stream_t stream);

/* Full-row GEMM with the residual add and the FOLLOWING LayerNorm fused (N = 768: csrc/gemm_frd.hip, or its 64-row twin
 * csrc/gemm_fr64.hip under "fr_tile" 64 — 64 <= M < 128 always runs the 64-row twin, same fp32 bits;
 * N = 1024: csrc/gemm_fr64.hip; M >= 64 everywhere):
 *   out fp32 [M,N] = residual + A[M,K] W[N,K]^T + bias   (residual may alias out: the in-place stream update of
 *   src/components/DiT.py:148 / :155),   u bf16 [M,ldu] = LayerNorm(out) * gamma + beta  (eps 1e-5; the norm of :152 / the
 *   next block's :105).  gamma = beta = u = NULL: no LayerNorm output.  K % 64 == 0.
 *   W is NOT the nn.Linear image: it is packed stage-major, Wp[K/16][N][16] (Wp[s][n][j] = W[n][16 s + j]), so that
 *   each K-step's 24 / 32 KiB are contiguous (the kernel moves them by LDS-DMA in whole cache lines).
 *   The residual is read at the stride ldo.  Rows move in 16-byte pieces: DITTO_ERR_SHAPE unless lda % 8 == 0, lda >= K, ldo >= N,
 *   ldo % 4 == 0 ("fr_hb": % 8), and, with a LayerNorm output, ldu >= N, ldu % 8 == 0 ("fr_u_fp8": % 16); DITTO_ERR_ARG unless A, W,
 *   out, residual, u, bias, gamma and beta are 16-byte aligned. */
int ditto_gemm_ln_bf16(const void* A, int lda, const void* W, const float* bias, const float* residual, float* out,
                       int ldo, const float* gamma, const float* beta, void* u_bf16, int ldu, int M, int N, int K,
                       ditto_stream_t stream);

/* LayerNorm fused INTO the GEMM that consumes it (csrc/gemm_lnq.hip; the model path's norm2 + cross-attention q-projection,
 * src/components/DiT.py:142-145; d = 768, or 1024 = BASELINE config C5):  out bf16 [M, ldo] = (LayerNorm(h) * gamma + beta)
 * W[d, d]^T + bias, eps 1e-5; the normalised rows live in the LDS only.  h: fp32 [M, ldh] or (h_is_bf16, d = 768) bf16 [M, ldh];
 * W: bf16, nn.Linear layout [d out, d in]; bias may be NULL.  mfma_shape 32 / 16 = v_mfma_f32_32x32x16_bf16 / 16x16x32 (two
 * builds of one kernel; d = 1024: 32 only).  w_scratch: d * d * 2 bytes, 256-byte aligned: receives the stage-major image of W the kernel streams (the model keeps
 * these images in its arena).  Any M >= 1.  ldh % 4 == 0, ldo % 8 == 0; h (fp32: 16 bytes, bf16: 8), out, gamma, beta and bias
 * 16-byte aligned (DITTO_ERR_ARG otherwise). */
int ditto_gemm_lnq_bf16(const void* h, int ldh, int h_is_bf16, const float* gamma, const float* beta, const void* W,
                        const float* bias, void* out_bf16, int ldo, int M, int d, int mfma_shape, void* w_scratch,
                        ditto_stream_t stream);

/* Weight-gradient GEMM of the backward pass (csrc/gemm_tn.hip): out fp32 [Mo, No] = X[K, Mo]^T Y[K, No], both operands
 * K-major bf16 (rows = the contraction index, as activations and their gradients lie in memory), i.e. dW = dY^T X of
 * nn.Linear (what autograd computes for reference src/TrainDiTTO.py:90).  tile = 128 (128x128, two workgroups per CU) or
 * 256 (256x256, one per CU); k_splits > 1: the contraction is split, fp32 partial tiles are summed in slice order
 * (deterministic).  workspace: 256 + k_splits * Mo * No * 4 bytes (256 alone when k_splits <= 1), 256-byte aligned.
 * Mo, No, ldx, ldy multiples of 8.  DITTO_ERR_ARG for what the kernels cannot serve: ldx < Mo; ldy < No; X or Y not
 * 16-byte aligned (the tiles are staged 16 B per lane); out not 16-byte aligned when k_splits > 1 (the reduce stores 16 B
 * per lane); also ldo < No, and ldo != No when k_splits > 1.  DITTO_ERR_SIZE for a workspace that is too small. */
int ditto_gemm_tn_bf16(const void* X, int ldx, const void* Y, int ldy, float* out, int ldo, int Mo, int No, int K,
                       int k_splits, int tile, void* workspace, size_t workspace_bytes, ditto_stream_t stream);

/* Process-wide tuning switches (tests / experiments).  "gemm_tile": 0 = automatic choice between the three GEMM
 * tile structures, 128 (128x128) / 129 (persistent 256x128 ring) / 131 (128x256 ping-pong, two workgroups per CU) /
 * 256 (persistent 256x256) = force one.  Results are identical up to fp32 summation order.
 * "pp_mask": GEMM classes that take the ping-pong kernel (bit 0 cross q-proj, 1 cross out-proj, 2 final projection,
 * 3 fc2, 4 QKV + RoPE, 5 gated MLP; -1 = the built-in rule).
 * "fr_mask": N = d = 768 projections on the full-row kernel with the residual add and the following LayerNorm fused
 * (csrc/gemm_fr.hip): bit 0 = cross out-proj + norm3, bit 1 = fc2 + the next block's norm1.
 * "fr_class_rows": the full-row kernel sums over k in a different order than the tiled GEMMs, so an utterance's bits depend on
 * whether its launch took it — a function of the launch's row count (>= 136 tiles of 128 rows, or 176 .. 271 tiles of 64 rows
 * except the 16129 .. 16384 rows that round up to 64 tiles of 256: csrc/kernels.h fr_rule_rows, a measured rule).  A pinned
 * class that a launch cannot take (full-row kernels, fewer than 64 rows in the launch) is an error (DITTO_ERR_SHAPE), never a
 * silent change of class.  A caller that splits ONE batch
 * over several launches or GPUs sets this to the rows (B * N) of the unsplit batch: every launch then decides as that batch
 * would and sharding changes no bit (ditto_tts_amd/dist.py sample_sharded does).  0 (default) = each launch on its own rows.
 * "fr_tile": which N = 768 full-row kernel: 0 (default) / 130 = 128-row tiles with the weights fetched straight from L2 into
 * registers (csrc/gemm_frd.hip); 64 = 64-row tiles, two workgroups per CU (csrc/gemm_fr64.hip) for launches with
 * K <= "fr64_maxk".  Both produce the same fp32 result bit for bit; the LayerNorm output may differ in the last bf16 bit of a few
 * elements (other association of the row statistics).  "fr_stagger": start delay of a CU's second workgroup in the 64-row
 * kernel, 10 ns ticks.  (N = 1024 always runs csrc/gemm_fr64.hip.)
 * "fr_u_fp8": TEST HOOK: ditto_gemm_ln_bf16 at N = 1024 writes u as fp8 e4m3 bytes ([M, ldu] bytes), the form the fp8 linear
 * path's model forward uses for norm3.
 * "fr_hb": TEST HOOK: ditto_gemm_ln_bf16 at N = 768 takes `residual` and `out` as bf16 [M, ldo] (ldo % 8 == 0, 16-byte aligned):
 * the 128-row kernel's bf16 residual stream form, which the model path runs (launches the 64-row kernel would take are an error).
 * "fr_dgrad": training backward, the long-K dgrads (N = d = 768) on the same kernel: bit 0 = fc1|gate (K = 8d), bit 1 = QKV.
 * "train_flags": training-step A/B switches: bit 0 = the backward of the self-attention rotation (RoPE) as its own pass over
 * dq | dk instead of inside the attention backward's dq / dk epilogues (head_dim 64; other head dims always take the pass);
 * bit 1 = the fc2 dgrad GEMM and the gated MLP's derivative as two launches instead of one (the derivative as the GEMM's
 * epilogue, from 144 tiles of 256 x 256 on); bit 2 = the training forward's gated GEMM on the general epilogue instead of its
 * own straight-line instantiation; bit 3 = the gradient wrt a LayerNorm's output as fp32 instead of bf16 between the dgrad GEMM
 * and the LayerNorm backward; bit 4 = the tape's residual-stream rows as fp32 instead of bf16 (the bf16 stream exists where the
 * inference forward has it: d = 768, head_dim 64, the full-row kernel class).  The flags must not change between the forward
 * and the backward of one step.
 * "fr_rot": that kernel's K-loop rotation (tiles start their k sum at different places so that the workgroups of an XCD do
 * not all ask the L2 for the same weight lines at once): 0 = off, 1 = on in the model path with period = row tiles per
 * utterance (an utterance's bits do not depend on its place in the batch), > 1 = ditto_gemm_ln_bf16 rotates too, with that
 * period in 128-row tiles.
 * "pp_nb": tile width of the ping-pong kernel's plain epilogues: 0 = rule, 3 = 128x192, 4 = 128x256.
 * "pp_stagger": phase offset between the two workgroups of a CU in the ping-pong GEMM, 10 ns ticks (-1 = built-in rule).
 * "gemm_flags": bit mask for kernel experiments (bit 0 = relaxed tile-start wait, default on; bits 1, 2 are
 * DIAGNOSTIC timing switches that skip stores / the epilogue and produce WRONG results — tools/ only; bit 14 = 16384: the
 * persistent 256x256 kernel takes the round-3 tile switch instead of running its K loop flat over it — A/B, bit-identical
 * results either way).
 * "gemm_group": forced super-column width of the GEMM tile order (A/B tool; 0 = the built-in rule, which a sweep of
 * 3 / 4 / 6 / 12 / 24 at C2 B = 32 did not beat).
 * "residual_bf16": 1 = the residual stream h between the segments of a block lives in HBM as bf16 (fp32 only inside the
 * accumulators and the LayerNorm statistics) for launches of the full-row class at d = 768 / head_dim 64; 0 = fp32 stream.
 * The sampler state x and eps stay fp32 either way.  (DITTO_RESIDUAL_BF16 in the environment sets the initial value.)
 * "lnq_waves": 8 (default) / 4 = waves per workgroup of the fused norm2 + q-projection (bit-identical).
 * "lnq": norm2 fused into the cross-attention q-projection (csrc/gemm_lnq.hip) for launches of the full-row class at d = 768:
 * 0 = LayerNorm launch + tiled GEMM, 32 / 16 = fused, on that MFMA shape.  (DITTO_LNQ sets the initial value.)
 * "splitk_wgs": K-splitting of the long-K GEMMs (fc2, final projection) of small batches, with an ordered fp32 reduce.
 * 0 (default) = the low-latency CLASS: launches of at most 2048 rows (1-2 utterances at N = 1024) split by a rule that depends
 * on K only (K = 3072: 4 splits), so an utterance's bits are independent of its batch neighbours INSIDE the class; across the
 * class boundary they differ in the last bits (as across the full-row class boundary), and "fr_class_rows" pins this class too
 * (-11 % step time at C2 B = 1).  -1 = never split (rounds 1-3 default).  > 0 = the older explicit rule: a workgroup target
 * (256 was the measured choice), under which the K partition depends on the batch size.
 * "qkv_split" (default 3; 0 = off): the QKV GEMM's last 256 columns (v columns) as a second launch where the rest makes whole
 * rounds of 256 x 256 tiles on the CUs, for launches of at most that many rounds (d = 768: B = 8, 16 at N = 1024); bit-identical.
 * "ll_mask" (default 3): the other launch forms of the low-latency class, each a function of the class and of K / Skv only:
 * bit 0 = fc2's split-K finish also writes the next block's norm1 (no bit changes), bit 1 = the cross out-projection as two
 * K-splits whose finish writes norm3.  Bit 1 changes a summation order: it is part of what defines the class (pin it with
 * class_rows as usual).  (ABI 9's bit 2, split-KV attention, measured slower and was removed in ABI 10.)
 * "attn_generic_kib": TEST HOOK: scratch budget, in KiB, of the GEMM-composed attention (head_dim != 64, the causal entries):
 * the path runs as many (batch, head) pairs per launch as fit it, at least one.  Default 2097152 (2 GiB); values below 1 are
 * refused.  ditto_attention_workspace_bytes, ditto_attention_causal_workspace_bytes and the length predictor's workspace sizes
 * follow it, so query them after setting it. */
int ditto_set_option(const char* name, int value);
/* Reads a switch back (callers that change one temporarily restore what they found: ditto_tts_amd/hip.py batch_class). */
int ditto_get_option(const char* name, int* value);

/* Which launches of one DiT block (reference src/components/DiT.py:148+152, :155+:105) a forward over B utterances of N
 * frames runs on the full-row kernel, under the current "fr_mask" / "fr_class_rows" options: *outproj, *fc2 = 0 / 1.  Host
 * arithmetic only (no GPU call): the full-row kernel addresses its operands with 32-bit byte offsets, so each launch is
 * admitted on the row stride IT reads with (fc2: 4 * hidden_dim). */
int ditto_full_row_plan(const ditto_config* cfg, int B, int N, int* outproj, int* fc2);
/* the same question for a call made with `opts` (NULL: as above); *stream_bf16 (may be NULL) = 1 when that forward carries its
 * residual stream as bf16 (d = 768, head_dim 64, bf16 linears, both fused launches on the 128-row kernel) */
int ditto_full_row_plan_opts(const ditto_config* cfg, int B, int N, const ditto_call_opts* opts, int* outproj, int* fc2,
                             int* stream_bf16);

/* ---- either side of the loop -------------------------------------------------------
 * ditto_vq_argmin: VectorQuantizer.forward (src/components/VectorQuantizer.py:22-43): idx[r] = argmin_k
 *   ||latents[r] - codebook[k]||^2 in fp32, first minimum on ties (torch.argmin); latents fp32 [R,D], codebook
 *   fp32 [K,D], idx int64 [R], scratch fp32 [K].
 * ditto_embedding_gather: nn.Embedding lookup out[i] = table[ids[i]] (GPT-2 wte for z_text,
 *   src/model/SpeechGenerator.py:101-103); table fp32 [V,d], ids int64 [n]; an id outside [0,V) is clamped to the
 *   table (nn.Embedding raises on the host; a stream-ordered kernel must not fault).
 * ditto_code_embed_mean: EnCodec codes -> embedding_head rows, mean over the C codebooks, first Fout frames
 *   (src/components/EnCodec.py:35-37, src/model/SpeechGenerator.py:97-98); codes int64 [B,C,F] -> fp32 [B,Fout,d].
 * ditto_linear_update: x <- a[b]*x + ce[b]*eps + cz[b]*noise (noise may be NULL): one step of a strided-DDPM /
 *   DDIM sampler (the paper's 25-step schedule; the reference only has stride 1).  a/ce/cz fp32 [B] (device).
 * ditto_cfg_combine: classifier-free guidance eps = eps_u + w*(eps_c - eps_u); eps2 fp32 [2,B,...] = [cond; uncond]. */
int ditto_vq_argmin(const float* latents, const float* codebook, int64_t* idx, int R, int K, int D, float* scratch_k,
                    ditto_stream_t stream);
int ditto_embedding_gather(const float* table, const int64_t* ids, float* out, int n, int V, int d,
                           ditto_stream_t stream);
int ditto_code_embed_mean(const float* table, const int64_t* codes, float* out, int B, int C, int F, int Fout, int V,
                          int d, ditto_stream_t stream);
int ditto_linear_update(float* x, const float* eps, const float* noise, const float* a, const float* ce,
                        const float* cz, int B, size_t elems_per_utt, ditto_stream_t stream);
int ditto_cfg_combine(const float* eps2, float* out, float w, size_t elems_half, ditto_stream_t stream);
/* Guided strided (DDIM) step over a variable-length batch (the paper's serving configuration: 25 steps, guidance 5.0).
 * ditto_guided_update: one launch for the update of a step.  x2, eps2 fp32 [2B, N, d] when cfg != 0 ([conditional; unconditional]:
 *   the forward over [text; null]), [B, N, d] when cfg == 0.  For utterance b < B, row r < speech_len[b]:
 *     e = cfg ? w[b] (c - u) + u : c  (c = eps2[b], u = eps2[B + b]: ditto_cfg_combine's fmaf),
 *     x' = a[b] x + ce[b] e + cz[b] z  (ditto_linear_update's fmaf order; z = cz = 0 with neither noise nor seeds),
 *   written to x2[b] and, when cfg != 0, to x2[B + b] (the next step's doubled input needs no copy).  Rows r >= speech_len[b] become 0
 *   in both halves without x, eps2 or the noise being read there; speech_len NULL = every row valid (device int32 [B], clamped into
 *   [1, N]).  The step's z: `noise` fp32 [B, N, d], or Philox from `seeds` (device int64 [B]) at tag `step`, the bits of
 *   ditto_noise_normal(seeds, step) on every valid row; giving both is DITTO_ERR_ARG.  w, a, ce, cz: device fp32 [B] (w only when
 *   cfg != 0; cz only with noise or seeds).  d % 64 == 0 (DITTO_ERR_SHAPE otherwise).
 * ditto_guided_step_opts: the forward over the B (cfg == 0) or 2B utterances of x2 with t int64 [2B or B], then
 *   ditto_guided_update into the same x2: one library call per step.  `cond` holds the 2B (or B) utterances' conditioning.  With
 *   speech_len and text_len both NULL the forward is ditto_forward_opts'; otherwise both are device int32 [2B or B] (every row of
 *   x2, as ditto_forward_varlen_opts takes them, and the conditioning from ditto_text_precompute_varlen with that text_len).
 *   The workspace is ditto_workspace_bytes(cfg, 2B or B, N, T). */
int ditto_guided_update(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                        const float* a, const float* ce, const float* cz, const int32_t* speech_len, int B, int N, int d, int cfg,
                        ditto_stream_t stream);
int ditto_guided_step_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* speech_len,
                           const int32_t* text_len, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                           const float* a, const float* ce, const float* cz, int B, int N, int T, int cfg, const float* rope_cos,
                           const float* rope_sin, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                           const ditto_call_opts* opts);

/* ---- Packed batches (flash-attention's varlen layout): utterances concatenated along the rows, no padding.  Utterance b owns speech
 * rows [cu_speech[b], cu_speech[b+1]) of x / eps [S, d] and text rows [cu_text[b], cu_text[b+1]) of text [S_T, text_dim]; RoPE
 * positions and the text mean-pool are local to the utterance, so utterance b is x[cu[b]:cu[b+1]] with text[cu_t[b]:cu_t[b+1]].
 * cu_speech / cu_text: DEVICE int32 [B + 1].  Precondition (not checked: that would need a sync): they start at 0, increase strictly,
 * end at S / S_T, and no utterance is longer than max_N / max_T.  The kernels clamp every offset and length into the buffers, so a bad
 * value gives wrong rows but never an out-of-bounds access.  head_dim 64 and bf16 linear layers only (DITTO_ERR_SHAPE otherwise).
 * Every launch but the attention, the AdaLN entry and the QKV + RoPE epilogue is row-wise and runs over the S rows as they are; the
 * full-row GEMMs run unrotated (as varlen).  Under the same kernel class (ditto_call_opts.class_rows) an utterance gets the bits of
 * the padded varlen path (ditto_forward_varlen_opts) — it serves the same reference calls, DiTTO.forward and sample_guided.
 * ditto_packed_workspace_bytes / ditto_packed_cond_bytes: the sizes for B utterances of S speech and S_T text rows (0 on a bad
 *   argument).  ditto_text_precompute_packed: text fp32 [S_T, text_dim] -> cond (K/V rows [S_T, ...] | tmod [B, 2d]).
 * ditto_forward_packed_opts: DiTTO.forward -> eps_out fp32 [S, d]; rope_cos / rope_sin: ditto_rope_tables(max_N) (used only under
 *   the A/B table flag of the QKV epilogue). */
size_t ditto_packed_workspace_bytes(const ditto_config* cfg, int B, int S, int S_T);
size_t ditto_packed_cond_bytes(const ditto_config* cfg, int B, int S_T);
int ditto_text_precompute_packed(ditto_model_t m, const float* text, const int32_t* cu_text, int B, int S_T, int max_T, void* cond,
                                 size_t cond_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream);
int ditto_forward_packed_opts(ditto_model_t m, const float* x, const void* cond, const int64_t* t, const int32_t* cu_speech,
                              const int32_t* cu_text, int B, int S, int max_N, int S_T, int max_T, const float* rope_cos,
                              const float* rope_sin, float* eps_out, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                              const ditto_call_opts* opts);
/* Unit entries of the packed attention (as ditto_attention_varlen_bf16 / ditto_attention_resid_varlen_bf16): q / out / resid rows
 * [cu_q[b], cu_q[b+1]) of Sq, k / v rows [cu_kv[b], cu_kv[b+1]) of Skv; max_q / max_kv bound the lengths.  Rows outside an
 * utterance's own range (other utterances' included) are never read or written.  An utterance gets the arithmetic of the padded
 * varlen kernel: the same bits. */
int ditto_attention_packed_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                                const int32_t* cu_q, const int32_t* cu_kv, int B, int H, int Sq, int Skv, int max_q, int max_kv, int dh,
                                ditto_stream_t stream);
int ditto_attention_resid_packed_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid_in,
                                      void* resid_out, int ldr, int resid_is_bf16, const int32_t* cu_q, const int32_t* cu_kv, int B, int H,
                                      int Sq, int Skv, int max_q, int max_kv, int dh, ditto_stream_t stream);
/* ditto_guided_update over a packed batch (sample_guided): x2, eps2 fp32 [S, d], or [2S, d] when cfg != 0 (rows [0, S)
 *   conditional, [S, 2S) unconditional), utterance b < B owning rows [cu[b], cu[b+1]) of each half (cu: device int32 [B + 1]).  The
 *   same expressions; the Philox quad index is utterance-local, ((row - cu[b]) d + col) / 4, so the step's z is
 *   ditto_noise_normal(seeds, step)'s; `noise` is packed fp32 [S, d].  No padding, nothing zeroed.
 * ditto_guided_step_packed_opts: the forward over x2's 2B (cfg) or B packed utterances, then that update: cu_speech device int32
 *   [2B + 1] over the 2S rows of [x; x] (= [cu; S + cu[1:]]) or [B + 1]; cu_text the conditioning's (ditto_text_precompute_packed
 *   over [text; null]); t int64 [2B or B].  Workspace: ditto_packed_workspace_bytes(cfg, 2B or B, 2S or S, S_T). */
int ditto_guided_update_packed(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                               const float* a, const float* ce, const float* cz, const int32_t* cu, int B, int S, int max_N, int d,
                               int cfg, ditto_stream_t stream);
int ditto_guided_step_packed_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                  const int32_t* cu_text, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                                  const float* a, const float* ce, const float* cz, int B, int S, int max_N, int S_T, int max_T, int cfg,
                                  const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                  ditto_stream_t stream, const ditto_call_opts* opts);

/* ---- Continuous batching over packed batches: utterances join and leave between steps, each at its own index of its own strided
 * schedule.  The reference's loop (src/model/SpeechGenerator.py:130-164: __p_sample and __sample_latents) serves one closed batch in
 * which every utterance starts at step 0 and runs the same steps; these entries serve the same per-utterance arithmetic to a batch
 * whose membership changes.
 * ditto_guided_update_packed_tags / ditto_guided_step_packed_tags_opts: ditto_guided_update_packed / ditto_guided_step_packed_opts
 *   with the Philox step tag of utterance b read from tags[b] (device uint32 [B]; may be NULL without seeds) instead of one scalar:
 *   utterance b gets the bits the scalar-tag entry gives it at step = tags[b].  An utterance with cz[b] == 0 (a sigma = 0 step of
 *   its schedule) gets the value of the entry called without noise (up to the sign of a zero).  Every other argument as there. */
int ditto_guided_update_packed_tags(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                    const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu, int B, int S,
                                    int max_N, int d, int cfg, ditto_stream_t stream);
int ditto_guided_step_packed_tags_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                       const int32_t* cu_text, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                       const float* w, const float* a, const float* ce, const float* cz, int B, int S, int max_N,
                                       int S_T, int max_T, int cfg, const float* rope_cos, const float* rope_sin, void* workspace,
                                       size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
/* ---- Speech prompts (zero-shot voice cloning): the first prompt_len[b] rows of utterance b are the target speaker's clean latents,
 * placed in front of the frames to generate.  The forward sees them like any other rows; the update leaves them alone.  The reference
 * has no prompting: like the strided loop and the guidance, this is pinned by its own formulas.
 * ditto_guided_update_packed_prompt / ditto_guided_update_packed_tags_prompt: ditto_guided_update_packed / _tags over rows
 *   [cu[b] + P_b, cu[b+1]) only, P_b = prompt_len[b] (device int32 [B], shared by both halves under cfg) clamped into [0, n_b - 1] on
 *   the device: a bad value gives wrong rows, never an access outside the buffers.  The prompt rows of x2 (both halves) and of eps2
 *   are neither read nor written.  The Philox quad index is local to the generated rows, ((row - cu[b] - P_b) d + col) / 4: a
 *   prompted utterance draws what an unprompted one of n_b - P_b rows draws, and prompt_len all 0 is the unprompted entry bit for
 *   bit.  `noise` stays packed [S, d] like x (its prompt rows are not read).
 * ditto_guided_step_packed_prompt_opts / ditto_guided_step_packed_tags_prompt_opts: the step entries with that update; the forward
 *   is unchanged. */
int ditto_guided_update_packed_prompt(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step,
                                      const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                      const int32_t* prompt_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream);
int ditto_guided_update_packed_tags_prompt(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                           const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                           const int32_t* prompt_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream);
int ditto_guided_step_packed_prompt_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                         const int32_t* cu_text, const int32_t* prompt_len, const float* noise, const int64_t* seeds,
                                         uint32_t step, const float* w, const float* a, const float* ce, const float* cz, int B, int S,
                                         int max_N, int S_T, int max_T, int cfg, const float* rope_cos, const float* rope_sin,
                                         void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
int ditto_guided_step_packed_tags_prompt_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                              const int32_t* cu_text, const int32_t* prompt_len, const float* noise, const int64_t* seeds,
                                              const uint32_t* tags, const float* w, const float* a, const float* ce, const float* cz,
                                              int B, int S, int max_N, int S_T, int max_T, int cfg, const float* rope_cos,
                                              const float* rope_sin, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                                              const ditto_call_opts* opts);
/* ---- Second-order multistep solver, DPM-Solver++(2M) (Lu et al. 2022), over packed batches: one forward per step like the strided
 * (DDIM) step, with the previous step's x0 prediction kept per generated row in `q` fp32 [S, d] (one half only).  Deterministic: no
 * noise.  The reference has neither solver: like the strided loop this is pinned by its own formulas (sampler.multistep_schedule).
 * ditto_multistep_coef: one utterance's step — per element
 *     e  = cfg ? w (c - u) + u : c          (ditto_guided_update's fmaf)
 *     x0 = fmaf(kx, x, ke e)                (kx = 1 / alpha, ke = -sigma / alpha)
 *     x' = fmaf(a, x, fmaf(b, x0, use_prev ? g q : 0)),   q = x0
 *   x' goes to both halves of x2 under cfg.  With use_prev == 0, q is written and NOT read (an utterance's first step meets an
 *   uninitialised history).
 * ditto_multistep_update_packed: the update alone.  Exactly one of `step` (a HOST pointer: the step every utterance stands at; its w
 *   is ignored and w[b], device fp32 [B], is the guidance scale under cfg) and `coefs` (DEVICE [B], 16-byte aligned: utterance b at
 *   coefs[b], guidance scale included; w is ignored) is given.  x2, eps2, cu, B, S, max_N, d, cfg: as ditto_guided_update_packed.
 *   prompt_len: NULL, or device int32 [B] clamped as in ditto_guided_update_packed_prompt — the prompt rows of x2, eps2 and q are
 *   neither read nor written.
 * ditto_guided_step_packed_multistep_opts: ditto_guided_step_packed_prompt_opts with that update (the forward is unchanged). */
typedef struct ditto_multistep_coef {
    float a, kx, ke, b, g, w;
    int32_t use_prev;
    int32_t reserved;  /* 0 */
} ditto_multistep_coef;
int ditto_multistep_update_packed(float* x2, const float* eps2, float* q, const ditto_multistep_coef* step,
                                  const ditto_multistep_coef* coefs, const float* w, const int32_t* cu, const int32_t* prompt_len,
                                  int B, int S, int max_N, int d, int cfg, ditto_stream_t stream);
int ditto_guided_step_packed_multistep_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                            const int32_t* cu_text, const int32_t* prompt_len, float* q,
                                            const ditto_multistep_coef* step, const ditto_multistep_coef* coefs, const float* w, int B,
                                            int S, int max_N, int S_T, int max_T, int cfg, const float* rope_cos, const float* rope_sin,
                                            void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
/* ---- Guidance in a limited interval (Kynkaanniemi et al. 2024) over a request stream: classifier-free guidance is applied on a range
 * of noise levels only, so a step of the stream holds guided and unguided utterances side by side and only the guided ones need the
 * unconditional forward.  The reference has no guided sampler: like the strided loop this is pinned by its own formulas.
 * Layout of a step with G of the B utterances guided: x2, eps2 fp32 [S + S_G, d] — every utterance in rows [0, S), the guided ones'
 *   unconditional copies compacted behind them in rows [S, S + S_G) in batch order; cu device int32 [B + G + 1] = [cu; S + cu_G[1:]]
 *   (copy g owns rows [cu[B + g], cu[B + g + 1])); partner device int32 [B]: the copy of utterance b in [0, G), or -1.
 * ditto_guided_update_packed_mixed: ditto_guided_update_packed_tags_prompt per utterance — with a partner its cfg != 0 arithmetic
 *   (eps_u read at the copy's rows, x' written to b's rows and to the copy's), without one its cfg == 0 arithmetic (nothing behind
 *   row S is read or written).  w, a, ce, cz, tags, seeds: [B]; noise packed fp32 [S, d]; prompt_len NULL or device int32 [B].
 *   partner[b] is clamped into [-1, G - 1]; the copy's span has b's own length n_b and its first row is clamped into
 *   [S, S + S_G - n_b] (n_b > S_G: no copy, b is updated without guidance): a bad table gives wrong rows — a copy's span may run
 *   into the next copy's — never an access outside the buffers.  G == 0 needs S_G == 0 and the reverse.
 * ditto_guided_step_packed_mixed_opts: one packed forward over the B + G utterances of x2 — cond is ditto_text_precompute_packed
 *   over [text_0 .. text_{B-1}; null_g ..] with cu_text [B + G + 1], t int64 [B + G] with a copy's t its partner's — then that
 *   update.  Workspace: ditto_packed_workspace_bytes(cfg, B + G, S + S_G, S_T). */
int ditto_guided_update_packed_mixed(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                     const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                     const int32_t* partner, const int32_t* prompt_len, int B, int G, int S, int S_G, int max_N, int d,
                                     ditto_stream_t stream);
int ditto_guided_step_packed_mixed_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                        const int32_t* cu_text, const int32_t* partner, const int32_t* prompt_len, const float* noise,
                                        const int64_t* seeds, const uint32_t* tags, const float* w, const float* a, const float* ce,
                                        const float* cz, int B, int G, int S, int S_G, int max_N, int S_T, int max_T,
                                        const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                        ditto_stream_t stream, const ditto_call_opts* opts);
/* ---- Guidance rescale (Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4) for packed guided
 * sampling: at a strong scale the guided prediction e = u + w (c - u) has a much larger standard deviation than the conditional
 * prediction c; e is scaled back so that its per-utterance standard deviation matches that of c, blended by phi.  The reference has no
 * guided sampler: this is pinned by its own formula.  Per guided utterance b, over its GENERATED rows [cu[b] + P_b, cu[b+1]) and all d
 * columns only (c, u fp32; e_i = fmaf(w_b, c_i - u_i, u_i), the update kernels' expression):
 *     sigma_c, sigma_e   population standard deviations of c and e, mean and variance accumulated in fp64
 *     r = sigma_c / sigma_e,   s = 1 + phi_b (r - 1) in fp64,   s32 = (float)s          phi_b clamped into [0, 1] on the device
 *     coef_out[b] = coef_in[b] * s32                                                   one fp32 multiply
 *   s32 = 1 and coef_out[b] a bit copy of coef_in[b] where phi_b == 0, the utterance is unguided (partner[b] < 0), sigma_e^2 <= 0 or r
 *   is not finite; an unguided or phi_b == 0 utterance has none of its eps read.  Nothing is read outside the generated rows of the
 *   rescaled utterances.  x' is linear in e, so the update with the rescaled prediction is the EXISTING update with coef_out in the
 *   place of ce (strided update) or ke (2M update); the noise term cz z is not scaled.
 *   Bits: the sums are cut into partials of 4096 16-byte quads of the utterance's own generated region (a constant of the library),
 *   each in a fixed order, summed per utterance in an order that depends on its chunk count only — no atomics.  s32 of an utterance is a
 *   function of its own generated rows, w_b and phi_b: not of its position, its neighbours, B, S, max_N or the grid.
 * Layouts (those of the update entries): partner NULL — eps2 [2S, d], u at row offset S, G and S_G unused; partner device int32 [B] —
 *   eps2 [S + S_G, d], cu [B + G + 1], u at the copy's rows, everything clamped as in ditto_guided_update_packed_mixed.  prompt_len NULL
 *   or device int32 [B], clamped as in ditto_guided_update_packed_prompt.
 * ditto_guidance_rescale_bytes: the scratch of B utterances whose longest generated region is at most max_N rows (host arithmetic; 0 on
 *   a bad shape).  Layout, each part 256-byte aligned: [coef_out: B ditto_multistep_coef, or fp32 [B] at its start | scale fp32 [B] at
 *   byte al256(32 B) | the partials, 4 doubles per chunk].  A larger scratch is used in full; max_N only sizes the grid.
 * ditto_guidance_rescale_packed: the two launches alone over the caller's eps2.  Exactly one of coef_in (device fp32 [B], with w device
 *   fp32 [B]; coef_out is fp32 [B]) and coefs (device ditto_multistep_coef [B], 16-byte aligned: w and ke inside; coef_out is a copy of
 *   the structs with ke scaled) is given.  phi device fp32 [B]; scratch 256-byte aligned, >= ditto_guidance_rescale_bytes(B, max_N, d).
 * ditto_guided_step_packed_rescale_opts: the forward, the rescale, then the existing update with ce s32 — chosen as the existing entries
 *   choose it: partner NULL: ditto_guided_step_packed_opts with cfg 1 (tags NULL: the scalar `step`), its _tags, _prompt or
 *   _tags_prompt form by tags / prompt_len; partner given: ditto_guided_step_packed_mixed_opts (tags needed with seeds).
 * ditto_guided_step_packed_multistep_rescale_opts: ditto_guided_step_packed_multistep_opts with cfg 1 and device coefs [B], ke s32. */
size_t ditto_guidance_rescale_bytes(int B, int max_N, int d);
int ditto_guidance_rescale_packed(const float* eps2, const float* w, const float* phi, const float* coef_in,
                                  const ditto_multistep_coef* coefs, const int32_t* cu, const int32_t* prompt_len, const int32_t* partner,
                                  int B, int G, int S, int S_G, int max_N, int d, void* scratch, size_t scratch_bytes,
                                  ditto_stream_t stream);
int ditto_guided_step_packed_rescale_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                          const int32_t* cu_text, const int32_t* partner, const int32_t* prompt_len, const float* noise,
                                          const int64_t* seeds, uint32_t step, const uint32_t* tags, const float* w, const float* phi,
                                          const float* a, const float* ce, const float* cz, int B, int G, int S, int S_G, int max_N,
                                          int S_T, int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                          size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                          const ditto_call_opts* opts);
int ditto_guided_step_packed_multistep_rescale_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                    const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len, float* q,
                                                    const ditto_multistep_coef* coefs, const float* phi, int B, int S, int max_N, int S_T,
                                                    int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                                    size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                                    const ditto_call_opts* opts);
/* Span-masked training over a packed batch with prompts (cu, prompt_len and their clamp as above; every buffer fp32 [S, d]).  z is
 *   either `noise`, a packed buffer whose prompt rows are not read, or Philox of (seeds[b], tag) at the generated-local quad index:
 *   exactly one of the two is given.
 * ditto_span_noise_packed: x_in = x0 on the prompt rows (a bit copy), fmaf(ca[b], x0, cs[b] z) on the generated rows; ca, cs device
 *   fp32 [B].
 * ditto_span_mse_packed: loss[0] = (1 / n_elems) sum over the generated rows of (eps - z)^2; grad_eps = (2 / n_elems) (eps - z) there
 *   and exactly 0 on the prompt rows, where eps is not read.  n_elems = d x the number of generated rows.  With seeds the noise is
 *   regenerated and never exists in memory.  No atomics: per-workgroup partial sums go to `workspace` (B x min(1024, ceil(max_N d /
 *   1024)) floats) and a second launch adds them in index order, so a repeated call gives the same bits. */
int ditto_span_noise_packed(const float* x0, const float* noise, const int64_t* seeds, uint32_t tag, const float* ca, const float* cs,
                            const int32_t* cu, const int32_t* prompt_len, float* x_in, int B, int S, int max_N, int d,
                            ditto_stream_t stream);
int ditto_span_mse_packed(const float* eps, const float* noise, const int64_t* seeds, uint32_t tag, const int32_t* cu,
                          const int32_t* prompt_len, size_t n_elems, float* grad_eps, float* loss, void* workspace,
                          size_t workspace_bytes, int B, int S, int max_N, int d, ditto_stream_t stream);
/* ---- Speech infilling: generate a WINDOW of each utterance with clean context on both sides.  The first P_b = prompt_len[b] and the
 * last Q_b = suffix_len[b] rows of utterance b are clean latents; the G_b = n_b - P_b - Q_b rows in between are generated.  The forward
 * sees context rows like any rows; the entries below leave them alone.  The reference has no such sampler: like the prompts this is
 * pinned by its own formulas.  Every entry is its _prompt / multistep / span counterpart with one more argument:
 *   suffix_len: device int32 [B], REQUIRED (NULL: DITTO_ERR_ARG), shared by both halves under cfg.  prompt_len: device int32 [B] or
 *   NULL (P = 0).  On the device P_b is clamped into [0, n_b - 1] and Q_b into [0, n_b - 1 - P_b]: at least one row is generated, and
 *   a bad value gives wrong rows, never an access outside the utterance's own rows.
 * Contract: with suffix_len all 0, every entry gives the bits of its counterpart on every buffer it writes — the loss and the partial
 *   sums of ditto_span_mse_window included.
 * ditto_guided_update_packed_window / ditto_guided_update_packed_tags_window: ditto_guided_update_packed_prompt / _tags_prompt over
 *   rows [cu[b] + P_b, cu[b+1] - Q_b) only.  Context rows of x2 (both halves), of eps2 and of `noise` are neither read nor written,
 *   on either side: 0 B per context element, 20 B per generated element under cfg.  The Philox quad index is local to the window,
 *   ((row - cu[b] - P_b) d + col) / 4: a windowed utterance draws what an unprompted one of G_b rows with the same seed draws.
 * ditto_guided_step_packed_window_opts / ditto_guided_step_packed_tags_window_opts: the step entries with that update; the forward is
 *   unchanged.
 * ditto_multistep_update_window / ditto_guided_step_packed_multistep_window_opts: ditto_multistep_update_packed /
 *   ditto_guided_step_packed_multistep_opts over the window; the context rows of q are untouched too.
 * ditto_span_noise_window / ditto_span_mse_window: ditto_span_noise_packed / ditto_span_mse_packed with the span anywhere: x_in is a
 *   bit copy of x0 on both context regions; grad_eps is exactly 0 on both and eps (and `noise`) is not read there; the Philox index
 *   is window-local; n_elems = d x sum of G_b.  The same walk, partial layout, workspace and reduction order as the counterparts. */
int ditto_guided_update_packed_window(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step,
                                      const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                      const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg,
                                      ditto_stream_t stream);
int ditto_guided_update_packed_tags_window(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                           const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                           const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg,
                                           ditto_stream_t stream);
int ditto_guided_step_packed_window_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                         const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len,
                                         const float* noise, const int64_t* seeds, uint32_t step, const float* w, const float* a,
                                         const float* ce, const float* cz, int B, int S, int max_N, int S_T, int max_T, int cfg,
                                         const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                         ditto_stream_t stream, const ditto_call_opts* opts);
int ditto_guided_step_packed_tags_window_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                              const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len,
                                              const float* noise, const int64_t* seeds, const uint32_t* tags, const float* w,
                                              const float* a, const float* ce, const float* cz, int B, int S, int max_N, int S_T,
                                              int max_T, int cfg, const float* rope_cos, const float* rope_sin, void* workspace,
                                              size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
int ditto_multistep_update_window(float* x2, const float* eps2, float* q, const ditto_multistep_coef* step,
                                  const ditto_multistep_coef* coefs, const float* w, const int32_t* cu, const int32_t* prompt_len,
                                  const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream);
int ditto_guided_step_packed_multistep_window_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                   const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len,
                                                   const int32_t* suffix_len, float* q, const ditto_multistep_coef* step,
                                                   const ditto_multistep_coef* coefs, const float* w, int B, int S, int max_N, int S_T,
                                                   int max_T, int cfg, const float* rope_cos, const float* rope_sin, void* workspace,
                                                   size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
int ditto_span_noise_window(const float* x0, const float* noise, const int64_t* seeds, uint32_t tag, const float* ca, const float* cs,
                            const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, float* x_in, int B, int S,
                            int max_N, int d, ditto_stream_t stream);
int ditto_span_mse_window(const float* eps, const float* noise, const int64_t* seeds, uint32_t tag, const int32_t* cu,
                          const int32_t* prompt_len, const int32_t* suffix_len, size_t n_elems, float* grad_eps, float* loss,
                          void* workspace, size_t workspace_bytes, int B, int S, int max_N, int d, ditto_stream_t stream);
/* ditto_span_vloss_window: the span loss of a network that predicts v = alpha z - sigma x0 (Salimans & Ho 2022) instead of the noise,
 *   over the window of ditto_span_mse_window — except that suffix_len may be NULL here as prompt_len may (both NULL: the whole
 *   utterance).  Per generated element of utterance b: target = fmaf(ca[b], z, -(cs[b] x0)), diff = pred - target; loss[0] = (1 /
 *   n_elems) sum of lw[b] diff^2 and grad_pred = (2 / n_elems) lw[b] diff; grad_pred is exactly 0 on both context regions, where pred,
 *   x0 and `noise` are not read.  z: `noise` or Philox of (seeds[b], tag) at the window-local quad index, exactly one of the two, as
 *   above.  ca, cs: device fp32 [B], the pair ditto_span_noise_window noised x0 with (x_in = ca x0 + cs z, so ca^2 + cs^2 = 1 makes
 *   target the v of that x_in).  lw: device fp32 [B] per-utterance loss weights, or NULL (all 1): a timestep weighting such as
 *   min-SNR-gamma is one host line.  x0: fp32 [S, d], one stream more than the MSE reads (12 B per generated element with seeds, 16 B
 *   with `noise`).  The walk, the partial layout, the workspace size and the ordered two-launch reduction are ditto_span_mse_window's:
 *   no atomics, a repeated call gives the same bits.
 * Contract: with ca = 1, cs = 0, lw NULL and a finite x0, grad_pred, loss and the partials in `workspace` are bit-equal to
 *   ditto_span_mse_window's on the same pred / noise / seeds (fmaf(1, z, -0) = z).  The reference has no v objective: like the
 *   samplers above this is pinned by its own formulas. */
int ditto_span_vloss_window(const float* pred, const float* x0, const float* noise, const int64_t* seeds, uint32_t tag, const float* ca,
                            const float* cs, const float* lw, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len,
                            size_t n_elems, float* grad_pred, float* loss, void* workspace, size_t workspace_bytes, int B, int S,
                            int max_N, int d, ditto_stream_t stream);
/* ---- Guidance reuse (the "CFG cache" of FasterCache, Lv et al. 2024, without its frequency reweighting): the unconditional forward
 * runs at every k-th guided step only, and the steps in between reuse the last guidance direction delta = c - u:
 *     u + w (c - u) = c + (w - 1)(c - u)  ~  c_now + (w - 1) delta_last
 * so a reuse step costs the unguided step's forward.  The reference has no guided sampler: this is pinned by its own formulas.  What
 * the approximation does to the speech of a trained model is not measured by anything in this library.
 * delta: fp32 [S, d], row-aligned with the conditional half, REQUIRED.  mode: 1 = STORE (a refresh step), 2 = LOAD (a reuse step);
 *   anything else is DITTO_ERR_ARG.  w: device fp32 [B], REQUIRED.  The window [cu[b] + P_b, cu[b+1] - Q_b), its clamps and the
 *   window-local Philox index are ditto_guided_update_packed_window's, except that prompt_len and suffix_len may each be NULL (0 rows);
 *   context rows of x2, eps, delta, q and `noise` are neither read nor written.
 * ditto_guided_update_packed_reuse: the scalar-tag strided (DDIM) update.
 *   STORE: eps fp32 [2S, d].  dl = c - u, e = fmaf(w[b], dl, u), x' = fmaf(a[b], x, fmaf(ce[b], e, cz[b] z)); x' goes to both halves of
 *     x2 [2S, d] — the bits of ditto_guided_update_packed_window with cfg = 1 — and delta = dl on the window rows.  mirror must be 0.
 *   LOAD: eps fp32 [S, d], the conditional prediction alone.  e = fmaf(w[b] - 1.0f, delta, c), the same x' line and the same draw;
 *     x' goes to rows [0, S) of x2 and, when mirror != 0, to the same rows + S as well (x2 is [2S, d] then, [S, d] otherwise).  delta
 *     is read and never written.  With w[b] == 1, e == c exactly and x' is the cfg = 0 entry's.
 * ditto_multistep_update_packed_reuse: the same two modes in front of ditto_multistep_update_window's x0 / x' / q lines, in the host
 *   `step` form only (REQUIRED; its w is ignored, w[b] is the scale; use_prev as there).  STORE gives that entry's cfg = 1 bits on x2
 *   and q.
 * ditto_guided_step_packed_reuse_opts / ditto_guided_step_packed_multistep_reuse_opts: the forward, then that update on its output.
 *   STORE: ditto_guided_step_packed_opts' cfg = 1 forward — the 2B utterances of [x; x], cu_speech [2B + 1] over 2S rows, cond over
 *     [text; null], t int64 [2B], workspace ditto_packed_workspace_bytes(cfg, 2B, 2S, S_T).
 *   LOAD: the forward over the B conditional utterances alone — x2's first S rows, cu_speech [B + 1], cond over the text only (S_T and
 *     max_T its own), t int64 [B], workspace ditto_packed_workspace_bytes(cfg, B, S, S_T).
 * Traffic of the update per generated element: STORE 4 B more than the cfg = 1 update; LOAD 16 B (x, c, delta read, x' written: 4 B
 *   more than the cfg = 0 update) + 4 B with a noise buffer + 4 B with mirror + 8 B multistep history.
 * In a request stream every utterance follows its own refresh schedule: ditto_guided_update_packed_refresh and
 *   ditto_guided_step_packed_refresh_opts serve refreshing, reusing and plain utterances in one launch, over the layout of
 *   ditto_guided_update_packed_mixed.  They are declared and documented in include/ditto_refresh.h. */
int ditto_guided_update_packed_reuse(float* x2, const float* eps, float* delta, const float* noise, const int64_t* seeds, uint32_t step,
                                     const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                     const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, int mode,
                                     int mirror, ditto_stream_t stream);
int ditto_multistep_update_packed_reuse(float* x2, const float* eps, float* q, float* delta, const ditto_multistep_coef* step,
                                        const float* w, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                        int S, int max_N, int d, int mode, int mirror, ditto_stream_t stream);
int ditto_guided_step_packed_reuse_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                        const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len, float* delta,
                                        const float* noise, const int64_t* seeds, uint32_t step, const float* w, const float* a,
                                        const float* ce, const float* cz, int B, int S, int max_N, int S_T, int max_T, int mode,
                                        int mirror, const float* rope_cos, const float* rope_sin, void* workspace,
                                        size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
int ditto_guided_step_packed_multistep_reuse_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                  const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len,
                                                  const int32_t* suffix_len, float* q, float* delta, const ditto_multistep_coef* step,
                                                  const float* w, int B, int S, int max_N, int S_T, int max_T, int mode, int mirror,
                                                  const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                                  ditto_stream_t stream, const ditto_call_opts* opts);
/* ditto_regroup_packed: build the next packed batch from the current one plus the newcomers, in ONE launch driven by a DEVICE table
 *   of n_seg segments.  A segment moves `n` 16-byte units (every row of the state, the K/V cache and tmod is a whole number of them)
 *   to unit dst_off of destination buffer `dest` and, when dup_off != 0, also to dst_off + dup_off (a speech segment under CFG: the
 *   unconditional half).  kind 0: the units come from unit src_off of source buffer `source` — a survivor's rows of the current
 *   state or conditioning, a newcomer's freshly computed conditioning, a caller's x_T, or offsets the caller appended to the
 *   uploaded table itself (cu, doubled cu, cu_text; name the table's buffer as a source).  kind 1: "draw x_T" — unit i of the
 *   segment is Philox of seeds[aux] at tag 0xFFFFFFFF, quad index i: with one segment per utterance, the numbers
 *   ditto_noise_normal(seeds, 0xFFFFFFFF) writes for it.  A destination may be an output buffer receiving the rows of utterances that
 *   leave.  src / dst: HOST arrays of n_bufs (<= 6) device pointers (16-byte aligned; NULL = absent) and their sizes in bytes
 *   (< 2^36).  Every index, offset and length of the table is clamped into those sizes on the device: a bad table gives wrong rows,
 *   never an access outside the buffers.  Segments must not overlap a destination range another segment reads or writes.
 *   max_bytes: the longest segment (sizes the grid only).  Nothing synchronises.
 * ditto_regroup_cond_layout: the packed conditioning image of S_T text rows (ditto_packed_cond_bytes): bytes of one K/V row and the
 *   byte offset of tmod fp32 [B, 2d] behind the S_T K/V rows. */
typedef struct ditto_regroup_seg {
    int32_t kind;      /* 0: copy, 1: draw x_T */
    int32_t source;    /* kind 0: index into src */
    int32_t dest;      /* index into dst */
    int32_t aux;       /* kind 1: index into seeds */
    uint32_t src_off;  /* 16-byte units */
    uint32_t dst_off;
    uint32_t n;
    uint32_t dup_off;
} ditto_regroup_seg;
int ditto_regroup_packed(const ditto_regroup_seg* table, int n_seg, const void* const* src, const size_t* src_bytes, void* const* dst,
                         const size_t* dst_bytes, int n_bufs, const int64_t* seeds, int n_seeds, size_t max_bytes,
                         ditto_stream_t stream);
int ditto_regroup_cond_layout(const ditto_config* cfg, int S_T, size_t* kv_row_bytes, size_t* tmod_offset);

/* ---- training: the backward of DiTTO.forward, so that the reference's training closure
 * (src/TrainDiTTO.py:55-95: model.train(); loss = mse(model(x_t, text, t), noise); loss.backward()) runs on this
 * library.  Gradients are fp32, in the reference's parameter layout (one pointer per state_dict key, as
 * ditto_weights); bf16 operands / fp32 accumulation inside, deterministic (no atomics).  No gradient is produced
 * for x, text_emb (both come from frozen encoders in the reference, TrainDiTTO.py:66-73) or for the dead
 * blocks.i.attn.out_proj.* (never used by the forward, src/components/DiT.py:134-139).
 *
 * ditto_train_attach : packs the transposed bf16 weight copies the dgrad GEMMs read (dX = dY W) into a caller-owned
 *                      arena; call after ditto_model_create, i.e. after every optimizer step.
 * ditto_train_forward: DiTTO.forward in train mode — as ditto_forward, from raw text_emb (no cached cond), keeping the
 *                      activations in `tape`; dropout_p is nn.MultiheadAttention's cross-attention dropout
 *                      (src/components/DiT.py:90-91), its mask a counter-based hash of (seed, layer, b, h, i, j).
 * ditto_train_backward: consumes the tape, writes every gradient of `grads` (overwrites, does not accumulate). */
typedef struct ditto_layer_grads {
    float* norm1_weight;  float* norm1_bias;
    float* attn_in_proj_weight;  float* attn_in_proj_bias;
    float* norm2_weight;  float* norm2_bias;
    float* cross_in_proj_weight; float* cross_in_proj_bias;
    float* cross_out_proj_weight; float* cross_out_proj_bias;
    float* norm3_weight;  float* norm3_bias;
    float* mlp_fc1_weight; float* mlp_fc1_bias;
    float* gate_weight;    float* gate_bias;
    float* mlp_fc2_weight; float* mlp_fc2_bias;
} ditto_layer_grads;
typedef struct ditto_grads {
    float* t_embedding_weight;
    float* time_embed_0_weight; float* time_embed_0_bias;
    float* time_embed_2_weight; float* time_embed_2_bias;
    float* ada_time_mlp_weight; float* ada_time_mlp_bias;
    float* ada_text_mlp_weight; float* ada_text_mlp_bias;
    float* proj_in_weight;  float* proj_in_bias;
    float* proj_out_weight; float* proj_out_bias;
    float* unused_rotary_inv_freq;                                       /* a buffer, no gradient; keeps the layout of ditto_weights */
    const ditto_layer_grads* layers;                                     /* HOST array [num_layers] */
} ditto_grads;
size_t ditto_train_arena_bytes(const ditto_config* cfg);
size_t ditto_tape_bytes(const ditto_config* cfg, int B, int N, int T);
size_t ditto_train_workspace_bytes(const ditto_config* cfg, int B, int N, int T);
int ditto_train_attach(ditto_model_t m, const ditto_weights* w, void* train_arena, size_t train_arena_bytes,
                       ditto_stream_t stream);
int ditto_train_forward(ditto_model_t m, const float* x, const float* text, const int64_t* t, int B, int N, int T,
                        const float* rope_cos, const float* rope_sin, float dropout_p, uint64_t seed, float* eps_out,
                        void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream);
int ditto_train_backward(ditto_model_t m, const ditto_weights* w, const float* grad_eps, const float* x,
                         const int64_t* t, int B, int N, int T, const float* rope_cos, const float* rope_sin,
                         float dropout_p, uint64_t seed, const void* tape, size_t tape_bytes, const ditto_grads* grads,
                         void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* The same two calls with their options as an argument.  The forward RECORDS in the handle, against the tape's address, how it
 * wrote the tape (bf16 or fp32 residual-stream rows); the backward reads the tape as it was written — whatever the options say by
 * then — and fails (DITTO_ERR_ARG / _SHAPE) on a tape no forward of this handle wrote or one written for another (B, N, T). */
int ditto_train_forward_opts(ditto_model_t m, const float* x, const float* text, const int64_t* t, int B, int N, int T,
                             const float* rope_cos, const float* rope_sin, float dropout_p, uint64_t seed, float* eps_out,
                             void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                             const ditto_call_opts* opts);
int ditto_train_backward_opts(ditto_model_t m, const ditto_weights* w, const float* grad_eps, const float* x,
                              const int64_t* t, int B, int N, int T, const float* rope_cos, const float* rope_sin,
                              float dropout_p, uint64_t seed, const void* tape, size_t tape_bytes, const ditto_grads* grads,
                              void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts);
/* The backward in pieces, for a caller that overlaps the data-parallel gradient exchange with it (ditto_tts_amd/dist.py GradSync:
 * the reduce-scatter / all-gather of the layers already done runs on another stream while the layers below are computed): this
 * call runs layers layer_from, layer_from - 1, ..., layer_to (num_layers > layer_from >= layer_to >= 0) and writes THEIR gradients
 * (grads->layers[l]); the call with layer_from == num_layers - 1 also runs the head (proj_in / proj_out gradients), the call with
 * layer_to == 0 the tail (GlobalAdaLN, time embedding).  Successive calls, top layer first, on ONE stream with ONE workspace (it
 * carries the stream gradient between them) are bit-identical to ditto_train_backward, which is the call (num_layers - 1, 0).
 * ONE gradient crosses a piece boundary: grads->layers[l].mlp_fc2_bias is the column sum taken by the LayerNorm backward of layer
 * l + 1's norm1 (the fused fc2 + norm1 launch of the forward), so it is written by the piece that CONTAINS LAYER l + 1 — the call
 * with layer_to == l + 1 writes layers[l].mlp_fc2_bias as well, and a piece's own top layer's fc2 bias gradient was written by the
 * piece above it (the top layer's: by the call with layer_from == num_layers - 1 itself).  A caller that allocates, zeroes or
 * exchanges gradient buffers per piece must treat layers[layer_to - 1].mlp_fc2_bias as part of the piece (dist.py GradSync does). */
int ditto_train_backward_layers(ditto_model_t m, const ditto_weights* w, const float* grad_eps, const float* x,
                                const int64_t* t, int B, int N, int T, const float* rope_cos, const float* rope_sin,
                                float dropout_p, uint64_t seed, const void* tape, size_t tape_bytes, const ditto_grads* grads,
                                void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts,
                                int layer_from, int layer_to);
/* ---- training on PACKED variable-length batches.  The reference pads a training batch (src/utils/MLS.py:136-151) and lets every
 * utterance attend to its neighbours' padding and pool it into the AdaLN text vector (src/components/DiT.py:25-40, 131-148: no
 * key-padding mask); here utterance b owns speech rows [cu_speech[b], cu_speech[b+1]) of x / eps [S, d] and text rows
 * [cu_text[b], cu_text[b+1]) of text [S_T, text_dim] (device int32 [B + 1] each, validated by the caller, clamped by every kernel that
 * turns one into an address), and its rows of eps are what ditto_train_forward gives for it alone: attention over its own keys, the
 * text pool over its own text rows, RoPE positions from its own first row (rope tables: at least max_N rows), dropout mask = the
 * hash on stream b * H + h at the utterance-local (query, key) indices.  Gradients: of the caller's scalar loss over the S rows =
 * the sum of the per-utterance gradients (src/TrainDiTTO.py:55-95 one utterance at a time), no atomics.  head_dim 64, bf16 linears.
 * The tape and the workspace are per ROW: a buffer sized for (B, S, S_T) serves any batch that needs no more bytes. */
size_t ditto_tape_bytes_packed(const ditto_config* cfg, int B, int S, int S_T);
size_t ditto_train_workspace_bytes_packed(const ditto_config* cfg, int B, int S, int max_N, int S_T, int max_T);
int ditto_train_forward_packed_opts(ditto_model_t m, const float* x, const float* text, const int64_t* t, const int32_t* cu_speech,
                                    const int32_t* cu_text, int B, int S, int max_N, int S_T, int max_T, const float* rope_cos,
                                    const float* rope_sin, float dropout_p, uint64_t seed, float* eps_out, void* tape,
                                    size_t tape_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                                    const ditto_call_opts* opts);
/* layers layer_from .. layer_to as ditto_train_backward_layers (src/TrainDiTTO.py:82-88 loss.backward()); the whole backward is the
 * call (num_layers - 1, 0) */
int ditto_train_backward_packed_layers(ditto_model_t m, const ditto_weights* w, const float* grad_eps, const float* x, const int64_t* t,
                                       const int32_t* cu_speech, const int32_t* cu_text, int B, int S, int max_N, int S_T, int max_T,
                                       const float* rope_cos, const float* rope_sin, float dropout_p, uint64_t seed, const void* tape,
                                       size_t tape_bytes, const ditto_grads* grads, void* workspace, size_t workspace_bytes,
                                       ditto_stream_t stream, const ditto_call_opts* opts, int layer_from, int layer_to);
/* The handle keeps one small record per tape a forward wrote (how it was written), until a forward rewrites that tape or the caller
 * says the tape's backward is done / the buffer is gone (src/TrainDiTTO.py:82-95: one backward per forward).  Records never leave
 * wholesale: a backward that is still pending always finds its own. */
int ditto_train_tape_forget(ditto_model_t m, const void* tape);
/* the packed forms of ditto_attention_dropout_bf16 / ditto_attention_bwd_bf16 (nn.MultiheadAttention in train mode,
 * src/components/DiT.py:131-148, per utterance): q / out / dout / dq [Sq, ld], k / v / dk / dv [Skv, ld], utterance b's rows from
 * cu_q / cu_kv (device int32 [B + 1]), max_q / max_kv the longest lengths, lse fp32 [H, Sq] (log2 domain), q UNSCALED.  Rows outside
 * every utterance's range are neither read nor written.  rope_cos / rope_sin (both or neither; self-attention, cu_q == cu_kv): the
 * inverse half-split rotation of dq / dk (src/components/DiT.py:126-129) at the row's position inside its utterance, tables
 * fp32 [>= max_q, 32].  workspace >= ditto_attention_bwd_packed_workspace_bytes(B, H, Sq). */
size_t ditto_attention_bwd_packed_workspace_bytes(int B, int H, int Sq);
int ditto_attention_train_packed_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                                      float* lse_out, const int32_t* cu_q, const int32_t* cu_kv, int B, int H, int Sq, int Skv,
                                      int max_q, int max_kv, int dh, float scale, float dropout_p, uint64_t seed, int layer,
                                      ditto_stream_t stream);
int ditto_attention_bwd_packed_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dout, int lddo,
                                    const void* out, int ldo, const float* lse, void* dq, int lddq, void* dk, int lddk, void* dv,
                                    int lddv, const int32_t* cu_q, const int32_t* cu_kv, int B, int H, int Sq, int Skv, int max_q,
                                    int max_kv, int dh, float scale, float dropout_p, uint64_t seed, int layer, const float* rope_cos,
                                    const float* rope_sin, void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* building blocks of the backward, exported for unit parity tests:
 * ditto_layernorm_bwd: dx_accum fp32 [M,d] += LN'(dy); dgamma_dbeta fp32 [groups, 2d] (rows_per_group * groups = M;
 *   gamma may be NULL = ones; dx_accum or dgamma_dbeta may be NULL); scratch >= ditto_layernorm_bwd_scratch_bytes.
 * ditto_attention_bwd_bf16: dq/dk/dv bf16 from dout bf16 (layouts as ditto_attention_bf16), dropout as above. */
size_t ditto_layernorm_bwd_scratch_bytes(int rows_per_group, int groups, int d);
int ditto_layernorm_bwd(const float* dy, const float* x, const float* gamma, float* dx_accum, float* dgamma_dbeta,
                        void* scratch, size_t scratch_bytes, int rows_per_group, int groups, int d,
                        ditto_stream_t stream);
size_t ditto_attention_bwd_workspace_bytes(int B, int H, int Sq, int Skv, int dh);
/* lse == NULL: GEMM-composed backward (any head_dim % 64 == 0; `out` unused).  lse != NULL (head_dim 64): the fused
 * two-kernel backward; lse fp32 [B,H,Sq] from ditto_attention_dropout_bf16(lse_out) and `out` that call's output. */
int ditto_attention_bwd_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dout,
                             int lddo, const void* out, int ldo, const float* lse, void* dq, int lddq, void* dk, int lddk,
                             void* dv, int lddv, int B, int H, int Sq, int Skv, int dh, float scale, float dropout_p,
                             uint64_t seed, int layer, void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* training-forward attention: as ditto_attention_bf16 with dropout.  lse_out == NULL: the GEMM-composed path;
 * lse_out != NULL (head_dim 64): the fused kernel, which also writes the log2-domain log-sum-exp per query row. */
int ditto_attention_dropout_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out,
                                 int ldo, float* lse_out, int B, int H, int Sq, int Skv, int dh, float scale,
                                 float dropout_p, uint64_t seed, int layer, void* workspace, size_t workspace_bytes,
                                 ditto_stream_t stream);
/* the RESIDUAL form of the training-forward attention (head_dim 64, q UNSCALED), as ditto_train_forward's self-attention launches it
 * (src/components/DiT.py:139: no out-projection): resid_out[row, h*64 + c] = resid_in[...] + O, resid_in == NULL = in place; the stream
 * is fp32 [rows, ldr] or (resid_bf16 = 1) bf16 [rows, ldr].  `out` (optional) receives O itself as bf16 [rows, ldo] beside the stream;
 * lse_out (required) the log2-domain log-sum-exp.  Dense (cu_q == cu_kv == NULL): rows = B * Sq / B * Skv, max_q == Sq, max_kv == Skv,
 * lse_out fp32 [B, H, Sq].  Packed (both given, device int32 [B + 1]): Sq / Skv are the rows of the buffers in all, max_q / max_kv the
 * longest lengths, lse_out fp32 [H, Sq], as ditto_attention_train_packed_bf16.  Every device pointer is followed by its byte size: the
 * extent the launch reads or writes in each buffer is computed on the host, and what does not fit is refused before any HIP call
 * (DITTO_ERR_SHAPE: dh != 64, a stride that is no multiple of 8 or narrower than H * 64, an extent out of range; then DITTO_ERR_ARG: a
 * null or misaligned pointer, a flag or dropout_p out of range, the bf16 stream / `out` / a packed batch under attn_flags 8192; then
 * DITTO_ERR_SIZE: a buffer shorter than its extent).  No arithmetic is added: one launch_attention, exported for unit parity tests. */
int ditto_attention_train_resid_bf16(const void* q, size_t q_bytes, int ldq, const void* k, size_t k_bytes, int ldk, const void* v,
                                     size_t v_bytes, int ldv, const void* resid_in, size_t resid_in_bytes, void* resid_out,
                                     size_t resid_out_bytes, int ldr, int resid_bf16, void* out, size_t out_bytes, int ldo,
                                     float* lse_out, size_t lse_out_bytes, const int32_t* cu_q, size_t cu_q_bytes, const int32_t* cu_kv,
                                     size_t cu_kv_bytes, int B, int H, int Sq, int Skv, int max_q, int max_kv, int dh, float scale,
                                     float dropout_p, uint64_t seed, int layer, ditto_stream_t stream);

/* fp8 building blocks, exported for unit parity tests (all e4m3, OCP):
 * ditto_quantize_rows_fp8: fp32 [rows, cols] -> fp8 [rows, cols] + scales fp32 [rows] (amax/448 per row);
 * ditto_layernorm_fp8: as ditto_layernorm_bf16 with a saturating fp8 result;
 * ditto_gemm_fp8: out = (A_fp8[M,K] * W_fp8[N,K]^T) * wscale[n] + bias ..., epilogue 0 (bf16), 1 (fp32 + residual),
 *                 4 (fp32), 5 (gated MLP, fp8 out [M, N/2], interleaved rows as epilogue 3). */
int ditto_quantize_rows_fp8(const float* src, int rows, int cols, void* dst_fp8, float* scales, ditto_stream_t stream);
int ditto_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* out_fp8, int M, int d,
                        ditto_stream_t stream);
int ditto_gemm_fp8(const void* A, int lda, const void* W, const float* wscale, const float* bias,
                   const float* residual, void* out, int ldo, int M, int N, int K, int epilogue,
                   ditto_stream_t stream);
/* Every fp8 GEMM launch as the model fills it (tests/test_gpu_gemm_fp8.py): ditto_gemm_epilogue_bf16's fields with fp8 e4m3
 * operands and wscale (fp32 [N], may be NULL = 1).  A, W and the gated output are bytes: lda, ldw and the gated ldo count bytes
 * (lda, ldw multiples of 16; the gated ldo a multiple of 8); every other stride as ditto_gemm_epilogue_bf16.  epilogue 0, 1, 4:
 * as ditto_gemm_fp8, with ldr, out2_bf16 / ldo2, ldw and w_rows; 2: QKV + RoPE, bf16 out (rope_* as ditto_gemm_epilogue_bf16);
 * 5: gated MLP, fp8 out [M, N / 2].  Any other epilogue (the packed RoPE, 9, included): DITTO_ERR_ARG, nothing launched.
 * *structure_out (may be NULL): 256 if a launch happened, 0 otherwise. */
int ditto_gemm_epilogue_fp8(const ditto_gemm_epilogue_args* args, const float* wscale, int epilogue, int* structure_out,
                            ditto_stream_t stream);

/* ---- the speech-length predictor's decoder stack ------------------------------------------
 * Second user of the GEMM / attention family: the nn.TransformerDecoder the reference builds at
 * src/model/SpeechLP.py:22-32 (post-norm layers, ReLU feed-forward, batch_first, no final norm) run as
 * src/model/SpeechLP.py:47-55 does in eval mode — causal boolean tgt_mask on the self-attention (:50,57-61), unmasked
 * cross-attention to the text memory (:52), then length_predictor on the LAST position (:54).  The pretrained encoders
 * in front of it (ByT5, EnCodec; :17-19,47-49) are out of scope: the entry point takes their outputs.
 * Weights: one pointer per state_dict key of `transformer.layers.{i}.*` / `length_predictor.*`, device fp32, row-major
 * as PyTorch stores them ([out, in]).  d_model and dim_feedforward must be multiples of 64; the head width
 * d_model / nhead is arbitrary (packed zero-padded to a multiple of 64, which changes no result). */
typedef struct ditto_slp_config {
    int32_t d_model, nhead, num_layers, dim_feedforward, num_classes;
} ditto_slp_config;
typedef struct ditto_slp_layer_weights {
    const float *self_in_proj_weight, *self_in_proj_bias;      /* self_attn.in_proj_weight [3d,d], .in_proj_bias [3d] */
    const float *self_out_proj_weight, *self_out_proj_bias;    /* self_attn.out_proj.weight [d,d], .bias [d] */
    const float *cross_in_proj_weight, *cross_in_proj_bias;    /* multihead_attn.in_proj_* */
    const float *cross_out_proj_weight, *cross_out_proj_bias;  /* multihead_attn.out_proj.* */
    const float *linear1_weight, *linear1_bias;                /* [dff,d], [dff] */
    const float *linear2_weight, *linear2_bias;                /* [d,dff], [d] */
    const float *norm1_weight, *norm1_bias, *norm2_weight, *norm2_bias, *norm3_weight, *norm3_bias;
} ditto_slp_layer_weights;
typedef struct ditto_slp_weights {
    const ditto_slp_layer_weights* layers;                     /* [num_layers] (host array of device pointers) */
    const float *length_predictor_weight, *length_predictor_bias;   /* [num_classes,d], [num_classes] */
} ditto_slp_weights;
typedef struct ditto_slp* ditto_slp_t;

size_t ditto_slp_arena_bytes(const ditto_slp_config* cfg);                       /* 0 + last_error on a bad config */
size_t ditto_slp_workspace_bytes(const ditto_slp_config* cfg, int B, int S, int T);
/* packs the weights (bf16, heads padded) into the caller's 256-byte aligned device arena */
int ditto_slp_create(const ditto_slp_config* cfg, const ditto_slp_weights* w, void* arena, size_t arena_bytes,
                     ditto_stream_t stream, ditto_slp_t* out);
void ditto_slp_destroy(ditto_slp_t m);
/* z_audio fp32 [B,S,d] (tgt), z_text fp32 [B,T,d] (memory) -> logits fp32 [B,num_classes];
 * decoded (optional, may be NULL): fp32 [B,S,d], the decoder output for every position (z_audio_decoded, :52). */
int ditto_slp_forward(ditto_slp_t m, const float* z_audio, const float* z_text, int B, int S, int T, float* logits,
                      float* decoded, void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* ---- variable-length batches ----
 * As ditto_slp_forward on a padded batch whose utterance b has audio_len[b] valid audio rows and text_len[b] valid text
 * rows (device int32 [B]; either may be NULL = all rows; values are clamped to [1, S] / [1, T] in the kernels):
 * logits[b] is what utterance b gives alone — the causal mask over its own positions, cross-attention over its own
 * text rows, length_predictor on its row audio_len[b] - 1.  The contents of the padding rows reach nothing, NaN and Inf
 * included.  decoded (optional): fp32 [B,S,d], rows at or past audio_len[b] exactly 0.
 * Without `decoded` and with the option "slp_last_row" at 1 (the default) the LAST layer computes K and V for all rows
 * and everything else for the B last rows only, its two attentions by the last-row kernel below; with 0 every layer
 * runs the GEMM-composed attention with lengths.  Workspace: ditto_slp_varlen_workspace_bytes (it depends on the
 * option "slp_lr_chunk": query it after setting that). */
size_t ditto_slp_varlen_workspace_bytes(const ditto_slp_config* cfg, int B, int S, int T);
int ditto_slp_forward_varlen(ditto_slp_t m, const float* z_audio, const float* z_text, const int32_t* audio_len,
                             const int32_t* text_len, int B, int S, int T, float* logits, float* decoded,
                             void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* the GEMM-composed attention with lengths on its own (unit tests): as ditto_attention_causal_bf16 with q_len / kv_len
 * (device int32 [B], either may be NULL) and `causal` 0 / 1.  Utterance b's query i sees keys
 * j < kv_len[b] (and, causal, j <= i + kv_len[b] - q_len[b]); output rows at or past q_len[b] are zero; k / v rows at or
 * past kv_len[b] and q rows at or past q_len[b] may hold anything.  Workspace: ditto_attention_causal_workspace_bytes. */
int ditto_attention_causal_varlen_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                                       void* out, int ldo, const int32_t* q_len, const int32_t* kv_len, int B, int H,
                                       int Sq, int Skv, int dh, float scale, int causal, void* workspace,
                                       size_t workspace_bytes, ditto_stream_t stream);
/* last-row attention on its own (unit tests): ONE query per (utterance, head), q bf16 [B, ldq], over keys
 * 0 .. len[b] - 1 of k / v bf16 [B * Skv, ldk / ldv] (len device int32 [B], clamped to [1, Skv]; NULL = Skv); out bf16
 * [B, ldo].  head_dim % 64 == 0, at most 2048; strides multiples of 8, q / k / v 16-byte aligned.  fp32 scores and
 * accumulation; the keys are split into chunks of "slp_lr_chunk" keys (ditto_get_option), one workgroup each, merged
 * in chunk order without atomics: the same bits every run.  Keys at or past len[b] are never loaded. */
size_t ditto_attention_last_row_workspace_bytes(int B, int H, int Skv, int dh);
int ditto_attention_last_row_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out,
                                  int ldo, const int32_t* len, int B, int H, int Skv, int dh, float scale,
                                  void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* the masked attention of that stack on its own (unit parity tests): as ditto_attention_bf16 with the causal mask
 * key j <= query i + (Skv - Sq); always the GEMM-composed path (any head_dim % 64 == 0, workspace required). */
size_t ditto_attention_causal_workspace_bytes(int B, int H, int Sq, int Skv, int dh);
int ditto_attention_causal_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                                void* out, int ldo, int B, int H, int Sq, int Skv, int dh, float scale,
                                void* workspace, size_t workspace_bytes, ditto_stream_t stream);
/* y = LayerNorm(x) * gamma + beta (eps 1e-5) as fp32 AND bf16 (post-norm residual stream + next GEMM operand);
 * either output may be NULL; y_f32 may alias x. */
int ditto_layernorm_dual(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_bf16, int M,
                         int d, ditto_stream_t stream);

/* ---- the forward row kernels on their own (unit tests: tests/test_gpu_rowwise.py) ----------------------------------
 * Each entry is one launch of csrc/rowwise.hip with every pointer of the launch visible; nothing is allocated and no
 * model handle is involved.  Every entry checks its arguments first: DITTO_ERR_ARG for a missing or misaligned pointer
 * (fp32 rows move as 16-byte pieces, bf16 rows as 8-byte pieces), DITTO_ERR_SHAPE for a size the kernel cannot serve.
 *
 * ditto_adaln_rows: the GlobalAdaLN entry of the forward (src/components/DiT.py:23,34-39) over x fp32 [B * N, d]:
 *   h = LayerNorm(x) (no affine, eps 1e-5) * (1 + ttab[ts, :d] + tmod[b, :d]) + ttab[ts, d:] + tmod[b, d:],  b = row / N,
 *   ts = t[b] (device int64 [B], clamped into [0, steps)) or, t NULL, b itself (ttab then holds one row per utterance).
 *   ttab fp32 [steps, 2d], tmod fp32 [B, 2d].  h_out: fp32 [B * N, d], or bf16 when h_is_bf16.  raw_bf16 (optional): bf16(x)
 *   at row stride ldraw >= d, ldraw % 4 == 0.  u1_bf16 (optional, needs g1 and be1 fp32 [d]): LayerNorm(h) * g1 + be1 as bf16
 *   [B * N, d], from the fp32 h in registers (block 0's norm1, src/components/DiT.py:105).  d % 4 == 0, d <= 2048.
 * ditto_adaln_rows_packed: the same over S packed rows with b = utt[row] (device int32 [S], ditto_packed_row_map). */
int ditto_adaln_rows(const float* x, const float* ttab, const float* tmod, const int64_t* t, int steps, void* h_out,
                     int h_is_bf16, void* raw_bf16, int ldraw, const float* g1, const float* be1, void* u1_bf16, int B, int N,
                     int d, ditto_stream_t stream);
int ditto_adaln_rows_packed(const float* x, const float* ttab, const float* tmod, const int64_t* t, int steps,
                            const int32_t* utt, void* h_out, int h_is_bf16, void* raw_bf16, int ldraw, const float* g1,
                            const float* be1, void* u1_bf16, int S, int d, ditto_stream_t stream);
/* ditto_splitk_finish: out fp32 [M, N] = ((partial[0] + partial[1] + ... in index order) + bias[col]) + residual, each step one
 *   fp32 addition; partial fp32, split s at element offset s * stride (stride >= M * N, stride % 4 == 0); bias, residual optional;
 *   residual may alias out.  out2_bf16 (optional): bf16(out) at row stride ldo2 >= N, ldo2 % 4 == 0.  u_bf16 (optional, needs gamma
 *   and beta fp32 [N], N <= 2048): LayerNorm(out) * gamma + beta as bf16 at row stride ldu >= N, ldu % 4 == 0 — the finish and the
 *   LayerNorm that follows it as one launch, the same bits as ditto_splitk_finish without u followed by ditto_layernorm_bf16. */
int ditto_splitk_finish(const float* partial, int nsplit, size_t stride, const float* bias, const float* residual, float* out,
                        void* out2_bf16, int ldo2, const float* gamma, const float* beta, void* u_bf16, int ldu, int M, int N,
                        ditto_stream_t stream);
/* ditto_text_mod: the text half of GlobalAdaLN (src/components/DiT.py:19-22,27,31): pooled fp32 [B, dt] = the mean over the first
 *   T_b rows of text fp32 [B, T, dt] (T_b = text_len[b], device int32 [B] clamped into [1, T]; text_len NULL: T), then
 *   tmod fp32 [B, 2d] = wx [2d, dt] silu(pooled) + bx [2d].  Rows at or past T_b are not read.
 * ditto_text_mod_packed: the same with utterance b's rows at [cu_text[b], cu_text[b + 1]) of text fp32 [S_T, dt]
 *   (device int32 [B + 1]; lengths clamped into [1, max_T]). */
int ditto_text_mod(const float* text, const int32_t* text_len, const float* wx, const float* bx, float* pooled, float* tmod,
                   int B, int T, int dt, int d, ditto_stream_t stream);
int ditto_text_mod_packed(const float* text, const int32_t* cu_text, int S_T, int max_T, const float* wx, const float* bx,
                          float* pooled, float* tmod, int B, int dt, int d, ditto_stream_t stream);
/* ditto_time_table: the table ditto_model_create builds, ttab fp32 [steps, 2d] = wt silu(w2 silu(w0 emb[s] + b0) + b2) + bt
 *   (src/model/DiTTO.py:75-76, src/components/DiT.py:14-17,30); emb fp32 [steps, td], w0 / w2 fp32 [td, td], wt fp32 [2d, td].
 *   td <= 4096 (three vectors of td floats are staged in the LDS). */
int ditto_time_table(const float* emb, const float* w0, const float* b0, const float* w2, const float* b2, const float* wt,
                     const float* bt, float* ttab, int steps, int td, int d, ditto_stream_t stream);
/* ditto_packed_row_map: utt[r] = the last utterance b with cu[b] <= r (clamped into [0, B)), pos[r] = r - cu[utt[r]] clamped
 *   into [0, max_len); cu device int32 [B + 1], utt / pos device int32 [S]. */
int ditto_packed_row_map(const int32_t* cu, int B, int S, int max_len, int32_t* utt, int32_t* pos, ditto_stream_t stream);

/* ---- profiling aid (bench.py): per-kernel-class HIP-event timing -------------------------
 * When enabled on a handle, ditto_forward brackets every launch with hipEvents on `stream`
 * (eager only; do not enable while capturing a graph).  ditto_profile_read synchronises the
 * recorded events and returns, per class, launches and summed milliseconds since the last reset.
 * Independently, with DITTO_ROCTX=1 in the environment every launch of the path sits inside a roctx range named
 * after its class (roctxRangePushA / Pop from librocprofiler-sdk-roctx, loaded lazily), so `rocprofv3
 * --marker-trace --kernel-trace` separates e.g. the out-projection from fc2 although they share one kernel. */
enum { DITTO_KC_LAYERNORM = 0, DITTO_KC_GEMM_QKV, DITTO_KC_GEMM_QPROJ, DITTO_KC_GEMM_OUTPROJ, DITTO_KC_GEMM_GATED,
       DITTO_KC_GEMM_FC2, DITTO_KC_GEMM_FINAL, DITTO_KC_ATTN_SELF, DITTO_KC_ATTN_CROSS, DITTO_KC_ADALN,
       DITTO_KC_UPDATE, DITTO_KC_COUNT };
int ditto_profile_enable(ditto_model_t m, int enable);
int ditto_profile_read(ditto_model_t m, int32_t* launches /*[DITTO_KC_COUNT]*/, float* ms /*[DITTO_KC_COUNT]*/);
const char* ditto_kernel_class_name(int kc);

#ifdef __cplusplus
}
#endif
#endif /* DITTO_HIP_H */
