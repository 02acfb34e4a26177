/* ditto_train_rows.h — C-ABI of the backward pass's row kernels of libditto_hip.so (csrc/train.hip, csrc/train_packed.hip), one
 * launch sequence of ONE launcher per entry (csrc/train_rows_api.hip), so that the suite can hold each of them elementwise against
 * an fp64 reference (tests/train_rows_ref.py, tests/test_gpu_train_rows.py).  The training path itself calls the launchers; these
 * entries add no arithmetic.
 *
 * They live in their own header, beside include/ditto_hip.h and under its conventions (status codes, ditto_last_error, device
 * pointers owned by the caller, no allocation, no synchronisation, stream-ordered enqueues); DITTO_ABI_VERSION does not change
 * with them.
 *
 * Every entry takes, behind every device pointer, the BYTE SIZE of the buffer that stands there, and refuses — before any HIP
 * call, with ditto_last_error naming the entry and the argument — what its kernel cannot serve:
 *   DITTO_ERR_SHAPE   a dimension, stride, mode or flag outside what is stated below
 *   DITTO_ERR_ARG     a null pointer where one is required (or a given one where none may be), a misaligned pointer
 *   DITTO_ERR_SIZE    a buffer smaller than the extent the launch reads or writes there
 * in this order.  "Extent" below is in elements from the pointer; nothing outside it is read or written.  A pointer marked
 * "or NULL" is not looked at (its size neither) when NULL.  Alignments are of the pointer; the strides' rules keep every row
 * aligned.  All dimensions are >= 1 unless said otherwise.
 */
#ifndef DITTO_TRAIN_ROWS_H
#define DITTO_TRAIN_ROWS_H

#include "ditto_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- LayerNorm backward, residual-stream form (launch_ln_bwd_stream; the group form is ditto_layernorm_bwd of ditto_hip.h) ----
 * Per row r of x [rows, d]: mean, rstd = 1 / sqrt(var + 1e-5) (biased variance), xhat = (x - mean) rstd, g = dy * gamma,
 *   dx = rstd (g - mean(g) - xhat mean(g xhat));  dx_accum[r] += dx;  dx_bf16[r] = bf16(dx_accum[r]) (the value just written);
 *   dgamma = sum_r dy xhat;  dbeta = sum_r dy;  colsum = sum_r dx_accum (the values just written).
 * dy: fp32 (16-byte aligned) or, dy_bf16 = 1, bf16 (8-byte aligned) [rows, d], read whole.  x likewise with x_bf16; x_bf16 = 1 needs
 * dy_bf16 = 1.  gamma fp32 [d], 16-byte aligned, or NULL = ones.  dx_accum fp32 [rows, d], 16-byte aligned, read and written whole.
 * dx_bf16 bf16 [rows, d], 8-byte aligned, written whole.  dgamma, dbeta, colsum: fp32 [d] each, written whole, or NULL: not written.
 * scratch: ditto_layernorm_bwd_scratch_bytes(rows, 1, d) bytes, 16-byte aligned (written, then read).  d % 4 == 0, 4 <= d <= 2048. */
int ditto_bwd_ln_stream(const void* dy, size_t dy_bytes, int dy_bf16, const void* x, size_t x_bytes, int x_bf16, const float* gamma,
                        size_t gamma_bytes, float* dx_accum, size_t dx_accum_bytes, void* dx_bf16, size_t dx_bf16_bytes, float* dgamma,
                        size_t dgamma_bytes, float* dbeta, size_t dbeta_bytes, float* colsum, size_t colsum_bytes, void* scratch,
                        size_t scratch_bytes, int rows, int d, ditto_stream_t stream);

/* ---- GlobalAdaLN reductions per utterance of a packed batch (launch_adaln_bwd_packed) ----
 * dmod fp32 [B, 2d] = [sum dy xhat | sum dy] over the rows [cu[b], cu[b + 1]) of dy, x fp32 [S, d] (xhat as above, no affine).
 * dy, x: 16-byte aligned, S * d elements (rows outside every utterance are not read).  cu: DEVICE int32 [B + 1], 4-byte aligned; the
 * kernel clamps an utterance's first row into [0, S - 1] and its length into [1, min(max_len, S - first)].  max_len: the longest
 * utterance, 1 .. S (sizes the grid).  dmod: 4-byte aligned, B * 2d elements written.  scratch: ditto_bwd_adaln_packed_scratch_bytes
 * bytes, 16-byte aligned.  d % 4 == 0, 4 <= d <= 2048, B <= 65535. */
size_t ditto_bwd_adaln_packed_scratch_bytes(int max_len, int B, int d);   /* 0, with ditto_last_error set, for arguments outside the above */
int ditto_bwd_adaln_packed(const float* dy, size_t dy_bytes, const float* x, size_t x_bytes, const int32_t* cu, size_t cu_bytes, float* dmod,
                           size_t dmod_bytes, void* scratch, size_t scratch_bytes, int B, int S, int max_len, int d,
                           ditto_stream_t stream);

/* ---- gated-MLP derivative (launch_gated_bwd) ----
 * pre bf16 [M, 2F]: fc1 | gate pre-activations interleaved in blocks of 16 (columns [32q, 32q + 16) = a of outputs 16q .., the next
 * 16 = g of the same outputs); dact bf16 [M, F].  dpre bf16 [M, 2F] in the same column order:
 *   da = dact sigmoid(g) (Phi(a) + a phi(a)),   dg = dact a Phi(a) sigmoid(g) (1 - sigmoid(g)).
 * colsum fp32 [2F] = column sums of the bf16 values WRITTEN to dpre (the fc1 | gate bias gradients), with scratch of 256 * 2F floats;
 * both NULL: dpre only; one of them NULL is refused.  F % 16 == 0.  Every buffer 16-byte aligned, read / written whole. */
int ditto_bwd_gated(const void* dact, size_t dact_bytes, const void* pre, size_t pre_bytes, void* dpre, size_t dpre_bytes, float* colsum,
                    size_t colsum_bytes, void* scratch, size_t scratch_bytes, int M, int F, ditto_stream_t stream);

/* ---- column sums, two deterministic stages (launch_colsum_f32 / launch_colsum_bf16) ----
 * out fp32 [n] = sum over the M rows of x [M, ld] (fp32, or bf16 with x_bf16 = 1), columns < n.  Extent of x: (M - 1) * ld + n.
 * n % 4 == 0, ld % 4 == 0, ld >= n.  x: 16-byte aligned (fp32) or 8-byte aligned (bf16; the 16-byte loads are taken when x is 16-byte
 * aligned and n, ld are multiples of 8).  out: 4-byte aligned.  scratch: ditto_bwd_colsum_scratch_bytes(M, n) bytes (at most 256 n
 * floats), 16-byte aligned. */
size_t ditto_bwd_colsum_scratch_bytes(int M, int n);                      /* 0, with ditto_last_error set, for M < 1 or n < 1 */
int ditto_bwd_colsum(const void* x, size_t x_bytes, int x_bf16, float* out, size_t out_bytes, void* scratch, size_t scratch_bytes, int M,
                     int n, int ld, ditto_stream_t stream);

/* ---- the second stage alone (launch_reduce_partials) ----
 * out fp32 [n] = sum_c partial fp32 [chunks, n], in a fixed order.  Both 16-byte aligned (n >= 65536 with n % 4 == 0 and chunks <= 32
 * moves 16 bytes per lane), read / written whole.  chunks * n < 2^40. */
int ditto_bwd_reduce_partials(const float* partial, size_t partial_bytes, float* out, size_t out_bytes, int chunks, size_t n,
                              ditto_stream_t stream);

/* ---- batched bf16 transpose (launch_transpose_bf16) ----
 * For z < nz_o * nz_i: dst_z [cols, ldT] = transpose of src_z [rows, cols] (row stride ld), columns rows .. ldT - 1 of every dst row
 * written as ZERO; src_z = src + (z / nz_i) * s_o + (z % nz_i) * s_i, dst_z = dst + z * d_z (elements).
 * Extent of src: (nz_o - 1) s_o + (nz_i - 1) s_i + (rows - 1) ld + cols; of dst: (nz_o nz_i - 1) d_z + cols * ldT, ALL of it written.
 * ld, cols, s_o, s_i, d_z multiples of 8; ld >= cols; ldT a multiple of 64, >= rows; nz_o * nz_i <= 65535; more than one slice
 * needs d_z >= cols * ldT (slices of dst must not overlap); cols <= 64 * 65535.  src, dst 16-byte aligned. */
int ditto_bwd_transpose_bf16(const void* src, size_t src_bytes, void* dst, size_t dst_bytes, int rows, int cols, int ld, int ldT, int nz_o,
                             int nz_i, size_t s_o, size_t s_i, size_t d_z, ditto_stream_t stream);

/* ---- dropout softmax rows of the generic-head_dim attention (launch_softmax_drop_rows / launch_softmax_bwd_rows) ----
 * Row r of the stack belongs to the (batch, head) pair bh0 + r / rows_per_bh and is its query r % rows_per_bh; keep(r, j) is the
 * counter hash of (seed, layer, pair, query, j) against p_drop (oracle.hash_dropout_mask), always kept at p_drop = 0.
 *   drop_rows:  P[r, j]  = bf16( softmax_j(scale S[r, :Skv]) keep / (1 - p_drop) )
 *   rows:       dS[r, j] = bf16( p (dPd[r, j] keep / (1 - p_drop) - sum_j p dPd keep / (1 - p_drop)) scale ),  p = softmax_j(scale S[r, :Skv])
 * S, dPd fp32 [nrows, ld], 4-byte aligned: columns < Skv of every row are read, extent (nrows - 1) ld + Skv.  P, dS bf16 [nrows, ld],
 * 2-byte aligned: ALL ld columns of every row are written, columns Skv .. ld - 1 as zero.  1 <= Skv <= ld; layer, bh0 >= 0;
 * 0 <= p_drop < 1; scale finite. */
int ditto_bwd_softmax_drop_rows(const float* S, size_t S_bytes, void* P, size_t P_bytes, int nrows, int rows_per_bh, int Skv, int ld,
                                float scale, uint64_t seed, int layer, int bh0, float p_drop, ditto_stream_t stream);
int ditto_bwd_softmax_rows(const float* S, size_t S_bytes, const float* dPd, size_t dPd_bytes, void* dS, size_t dS_bytes, int nrows,
                           int rows_per_bh, int Skv, int ld, float scale, uint64_t seed, int layer, int bh0, float p_drop,
                           ditto_stream_t stream);

/* ---- the [B, .] affine maps of the modulation vectors, fp32 (launch_small_linear_fwd / _bwd_w / _bwd_x) ----
 * f = SiLU (silu_in = 1) or the identity (0).  x [B, I], W [O, I], dy [B, O], all contiguous, 4-byte aligned, read whole.
 *   mode 0 (fwd):    out [B, O] = f(x) W^T + bias.        dy must be NULL; bias fp32 [O] is READ, or NULL = none.
 *   mode 1 (bwd_w):  out [O, I] = dy^T f(x);  bias [O] = sum_b dy is WRITTEN, or NULL: not written.      W must be NULL.
 *   mode 2 (bwd_x):  out [B, I] = f'(x) * (dy W).         bias must be NULL; x is read only with silu_in = 1 and may be NULL without.
 * out is written whole.  B, O <= 65535. */
#define DITTO_SMALL_LINEAR_FWD 0
#define DITTO_SMALL_LINEAR_BWD_W 1
#define DITTO_SMALL_LINEAR_BWD_X 2
int ditto_bwd_small_linear(int mode, const float* x, size_t x_bytes, const float* W, size_t W_bytes, const float* dy, size_t dy_bytes,
                           float* out, size_t out_bytes, float* bias, size_t bias_bytes, int B, int I, int O, int silu_in,
                           ditto_stream_t stream);

/* ---- nn.Embedding backward (launch_embedding_scatter_add) ----
 * For b = 0 .. B - 1 in order: dtable[clamp(ids[b], 0, V - 1)] += drows[b]  (fp32 additions in b order; duplicates accumulate).
 * drows fp32 [B, d]; ids int64 [B], 8-byte aligned; dtable fp32 [V, d], read and written in the rows the ids name only. */
int ditto_bwd_embedding_scatter_add(const float* drows, size_t drows_bytes, const int64_t* ids, size_t ids_bytes, float* dtable,
                                    size_t dtable_bytes, int B, int V, int d, ditto_stream_t stream);

/* ---- packed-order packers and unpackers (launch_pack_bf16_t / launch_unpack_rows / launch_unpack_vec) ----
 * map(r) = (r / blk) * (blk * mult) + r % blk + row_off   (blk, mult >= 1, row_off >= 0; increasing in r).
 *   pack_bf16_t:  dst bf16 [cols, ldT]: dst[c][map(r)] = bf16(src[r][c]) for r < rows, c < cols; src fp32 [rows, cols] contiguous.
 *                 ldT > map(rows - 1).  Extent of dst: (cols - 1) ldT + map(rows - 1) + 1; the positions no map(r) reaches are
 *                 NOT written.  src 4-byte, dst 2-byte aligned.  cols <= 32 * 65535.
 *   unpack_rows:  dst fp32 [rows, cols] = src[map(r)][:], src fp32 [map(rows - 1) + 1, cols]; cols % 4 == 0; both 16-byte aligned.
 *   unpack_vec:   dst fp32 [rows] = src[map(r)], src fp32 [map(rows - 1) + 1]; 4-byte aligned. */
int ditto_bwd_pack_bf16_t(const float* src, size_t src_bytes, void* dst, size_t dst_bytes, int rows, int cols, int ldT, int blk, int mult,
                          int row_off, ditto_stream_t stream);
int ditto_bwd_unpack_rows(const float* src, size_t src_bytes, float* dst, size_t dst_bytes, int rows, int cols, int blk, int mult,
                          int row_off, ditto_stream_t stream);
int ditto_bwd_unpack_vec(const float* src, size_t src_bytes, float* dst, size_t dst_bytes, int rows, int blk, int mult, int row_off,
                         ditto_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
