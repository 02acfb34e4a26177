// train_rows_api.hip — the C entries of include/ditto_train_rows.h: one call of ONE launcher of train.hip / train_packed.hip each, every
// pointer and its byte size visible.  An entry computes, on the host and before any HIP call, the extent its launch reads or writes in
// every buffer and refuses what does not fit (DITTO_ERR_SHAPE, then DITTO_ERR_ARG, then DITTO_ERR_SIZE): a test that gets an argument or
// a buffer size wrong is answered here and never launched.  No arithmetic is added: the launchers are the ones the backward pass calls.
#include <math.h>

#include "../../include/ditto_train_rows.h"
#include "common.h"
#include "kernels.h"
#include "model.h"

namespace ditto {
namespace {

// (ArgBuf, check_bufs — one device buffer of an entry and its refusals: model.h)
bool ln_dim(int d) { return d >= 4 && d <= 2048 && d % 4 == 0; }
// the packed row of the last of `rows` rows, or -1 when the map's arguments are out of range or it leaves int
long long last_packed_row(int rows, int blk, int mult, int row_off) {
    if (rows < 1 || blk < 1 || mult < 1 || row_off < 0) return -1;
    const long long m = (long long)((rows - 1) / blk) * ((long long)blk * mult) + (rows - 1) % blk + row_off;
    return m > 0x7FFFFFFFLL - 1 ? -1 : m;
}

}  // namespace
}  // namespace ditto

using namespace ditto;

extern "C" {

int ditto_bwd_ln_stream(const void* dy, size_t dy_bytes, int dy_bf16, const void* x, size_t x_bytes, int x_bf16, const float* gamma,
                        size_t gamma_bytes, float* dx_accum, size_t dx_accum_bytes, void* dx_bf16, size_t dx_bf16_bytes, float* dgamma,
                        size_t dgamma_bytes, float* dbeta, size_t dbeta_bytes, float* colsum, size_t colsum_bytes, void* scratch,
                        size_t scratch_bytes, int rows, int d, ditto_stream_t stream) {
    const char* who = "ditto_bwd_ln_stream";
    if (rows < 1 || !ln_dim(d)) return fail(DITTO_ERR_SHAPE, "%s: rows %d, d %d: need rows >= 1, d %% 4 == 0, 4 <= d <= 2048", who, rows, d);
    if ((dy_bf16 | x_bf16) & ~1 || (x_bf16 && !dy_bf16))
        return fail(DITTO_ERR_SHAPE, "%s: dy_bf16 %d, x_bf16 %d: flags are 0 / 1 and a bf16 x needs a bf16 dy", who, dy_bf16, x_bf16);
    const size_t n = (size_t)rows * d, row = (size_t)d * 4;
    if (int rc = check_bufs(who, {{"dy", dy, dy_bytes, n * (dy_bf16 ? 2 : 4), dy_bf16 ? 8u : 16u, false},
                                  {"x", x, x_bytes, n * (x_bf16 ? 2 : 4), x_bf16 ? 8u : 16u, false},
                                  {"gamma", gamma, gamma_bytes, row, 16, true},
                                  {"dx_accum", dx_accum, dx_accum_bytes, n * 4, 16, false},
                                  {"dx_bf16", dx_bf16, dx_bf16_bytes, n * 2, 8, false},
                                  {"dgamma", dgamma, dgamma_bytes, row, 4, true},
                                  {"dbeta", dbeta, dbeta_bytes, row, 4, true},
                                  {"colsum", colsum, colsum_bytes, row, 4, true},
                                  {"scratch", scratch, scratch_bytes, ln_bwd_scratch_bytes(rows, 1, d), 16, false}}))
        return rc;
    HIP_TRY(launch_ln_bwd_stream(dy, dy_bf16 != 0, x, x_bf16 != 0, gamma, dx_accum, dx_bf16, dgamma, dbeta, colsum, (float*)scratch, rows, d,
                                 (hipStream_t)stream));
    return DITTO_OK;
}

size_t ditto_bwd_adaln_packed_scratch_bytes(int max_len, int B, int d) {
    if (max_len < 1 || B < 1 || B > 65535 || !ln_dim(d)) {
        fail(DITTO_ERR_SHAPE, "ditto_bwd_adaln_packed_scratch_bytes: max_len %d, B %d, d %d out of range", max_len, B, d);
        return 0;
    }
    return adaln_bwd_packed_scratch_bytes(max_len, B, d);
}
int ditto_bwd_adaln_packed(const float* dy, size_t dy_bytes, const float* x, size_t x_bytes, const int32_t* cu, size_t cu_bytes, float* dmod,
                           size_t dmod_bytes, void* scratch, size_t scratch_bytes, int B, int S, int max_len, int d,
                           ditto_stream_t stream) {
    const char* who = "ditto_bwd_adaln_packed";
    if (B < 1 || B > 65535 || S < 1 || max_len < 1 || max_len > S || !ln_dim(d))
        return fail(DITTO_ERR_SHAPE, "%s: B %d, S %d, max_len %d, d %d: need 1 <= B <= 65535, 1 <= max_len <= S, d %% 4 == 0, 4 <= d <= 2048",
                    who, B, S, max_len, d);
    const size_t n = (size_t)S * d * 4;
    if (int rc = check_bufs(who, {{"dy", dy, dy_bytes, n, 16, false},
                                  {"x", x, x_bytes, n, 16, false},
                                  {"cu", cu, cu_bytes, ((size_t)B + 1) * 4, 4, false},
                                  {"dmod", dmod, dmod_bytes, (size_t)B * 2 * d * 4, 4, false},
                                  {"scratch", scratch, scratch_bytes, adaln_bwd_packed_scratch_bytes(max_len, B, d), 16, false}}))
        return rc;
    HIP_TRY(launch_adaln_bwd_packed(dy, x, cu, B, S, max_len, d, dmod, (float*)scratch, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_bwd_gated(const void* dact, size_t dact_bytes, const void* pre, size_t pre_bytes, void* dpre, size_t dpre_bytes, float* colsum,
                    size_t colsum_bytes, void* scratch, size_t scratch_bytes, int M, int F, ditto_stream_t stream) {
    const char* who = "ditto_bwd_gated";
    if (M < 1 || F < 16 || F % 16 || F > (1 << 28)) return fail(DITTO_ERR_SHAPE, "%s: M %d, F %d: need M >= 1, F %% 16 == 0", who, M, F);
    if (!colsum != !scratch) return fail(DITTO_ERR_ARG, "%s: colsum and scratch are given together or both null", who);
    const size_t n = (size_t)M * F * 2;
    if (int rc = check_bufs(who, {{"dact", dact, dact_bytes, n, 16, false},
                                  {"pre", pre, pre_bytes, 2 * n, 16, false},
                                  {"dpre", dpre, dpre_bytes, 2 * n, 16, false},
                                  {"colsum", colsum, colsum_bytes, (size_t)2 * F * 4, 4, true},
                                  {"scratch", scratch, scratch_bytes, (size_t)256 * 2 * F * 4, 16, true}}))
        return rc;
    HIP_TRY(launch_gated_bwd(dact, pre, dpre, M, F, (hipStream_t)stream, colsum, (float*)scratch));
    return DITTO_OK;
}

size_t ditto_bwd_colsum_scratch_bytes(int M, int n) {
    if (M < 1 || n < 1) {
        fail(DITTO_ERR_SHAPE, "ditto_bwd_colsum_scratch_bytes: M %d, n %d must be positive", M, n);
        return 0;
    }
    return colsum_scratch_bytes(M, n);
}
int ditto_bwd_colsum(const void* x, size_t x_bytes, int x_bf16, float* out, size_t out_bytes, void* scratch, size_t scratch_bytes, int M,
                     int n, int ld, ditto_stream_t stream) {
    const char* who = "ditto_bwd_colsum";
    if (M < 1 || n < 4 || n % 4 || ld % 4 || ld < n || x_bf16 & ~1)
        return fail(DITTO_ERR_SHAPE, "%s: M %d, n %d, ld %d, x_bf16 %d: need M >= 1, n %% 4 == 0, ld %% 4 == 0, ld >= n", who, M, n, ld, x_bf16);
    const size_t esz = x_bf16 ? 2 : 4;
    if (int rc = check_bufs(who, {{"x", x, x_bytes, ((size_t)(M - 1) * ld + n) * esz, x_bf16 ? 8u : 16u, false},
                                  {"out", out, out_bytes, (size_t)n * 4, 4, false},
                                  {"scratch", scratch, scratch_bytes, colsum_scratch_bytes(M, n), 16, false}}))
        return rc;
    if (x_bf16) HIP_TRY(launch_colsum_bf16(x, ld, M, n, out, (float*)scratch, (hipStream_t)stream));
    else HIP_TRY(launch_colsum_f32((const float*)x, ld, M, n, out, (float*)scratch, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_bwd_reduce_partials(const float* partial, size_t partial_bytes, float* out, size_t out_bytes, int chunks, size_t n,
                              ditto_stream_t stream) {
    const char* who = "ditto_bwd_reduce_partials";
    if (chunks < 1 || n < 1 || n > ((size_t)1 << 34) || (size_t)chunks * n >= ((size_t)1 << 40))
        return fail(DITTO_ERR_SHAPE, "%s: chunks %d, n %zu: need chunks >= 1, 1 <= n <= 2^34, chunks * n < 2^40", who, chunks, n);
    if (int rc = check_bufs(who, {{"partial", partial, partial_bytes, (size_t)chunks * n * 4, 16, false},
                                  {"out", out, out_bytes, n * 4, 16, false}}))
        return rc;
    HIP_TRY(launch_reduce_partials(partial, chunks, n, out, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_bwd_transpose_bf16(const void* src, size_t src_bytes, void* dst, size_t dst_bytes, int rows, int cols, int ld, int ldT, int nz_o,
                             int nz_i, size_t s_o, size_t s_i, size_t d_z, ditto_stream_t stream) {
    const char* who = "ditto_bwd_transpose_bf16";
    const size_t lim = (size_t)1 << 40;
    if (rows < 1 || cols < 8 || cols % 8 || cols > 64 * 65535 || ld % 8 || ld < cols || ldT < 64 || ldT % 64 || ldT < rows)
        return fail(DITTO_ERR_SHAPE, "%s: rows %d, cols %d, ld %d, ldT %d: need cols, ld multiples of 8, ld >= cols, ldT a multiple of 64 >= rows",
                    who, rows, cols, ld, ldT);
    if (nz_o < 1 || nz_i < 1 || (long long)nz_o * nz_i > 65535 || s_o % 8 || s_i % 8 || d_z % 8 || s_o >= lim || s_i >= lim || d_z >= lim)
        return fail(DITTO_ERR_SHAPE, "%s: nz_o %d, nz_i %d, s_o %zu, s_i %zu, d_z %zu: need 1 <= nz_o * nz_i <= 65535, strides multiples of 8", who,
                    nz_o, nz_i, s_o, s_i, d_z);
    const size_t nz = (size_t)nz_o * nz_i, slice = (size_t)cols * ldT;
    if (nz > 1 && d_z < slice) return fail(DITTO_ERR_SHAPE, "%s: d_z %zu < cols * ldT = %zu: the slices of dst overlap", who, d_z, slice);
    const size_t src_ext = (size_t)(nz_o - 1) * s_o + (size_t)(nz_i - 1) * s_i + (size_t)(rows - 1) * ld + cols;
    if (int rc = check_bufs(who, {{"src", src, src_bytes, src_ext * 2, 16, false},
                                  {"dst", dst, dst_bytes, ((nz - 1) * d_z + slice) * 2, 16, false}}))
        return rc;
    HIP_TRY(launch_transpose_bf16(src, ld, rows, cols, dst, ldT, (hipStream_t)stream, nz_o, nz_i, (long long)s_o, (long long)s_i,
                                  (long long)d_z));
    return DITTO_OK;
}

static int softmax_rows_shape(const char* who, int nrows, int rows_per_bh, int Skv, int ld, float scale, int layer, int bh0, float p_drop) {
    if (nrows < 1 || rows_per_bh < 1 || Skv < 1 || ld < Skv || layer < 0 || bh0 < 0)
        return fail(DITTO_ERR_SHAPE, "%s: nrows %d, rows_per_bh %d, Skv %d, ld %d, layer %d, bh0 %d: need 1 <= Skv <= ld and no negative index", who,
                    nrows, rows_per_bh, Skv, ld, layer, bh0);
    if (!(p_drop >= 0.f && p_drop < 1.f) || !std::isfinite(scale))
        return fail(DITTO_ERR_SHAPE, "%s: p_drop %g outside [0, 1) or scale %g not finite", who, p_drop, scale);
    return DITTO_OK;
}
int ditto_bwd_softmax_drop_rows(const float* S, size_t S_bytes, void* P, size_t P_bytes, int nrows, int rows_per_bh, int Skv, int ld,
                                float scale, uint64_t seed, int layer, int bh0, float p_drop, ditto_stream_t stream) {
    const char* who = "ditto_bwd_softmax_drop_rows";
    if (int rc = softmax_rows_shape(who, nrows, rows_per_bh, Skv, ld, scale, layer, bh0, p_drop)) return rc;
    if (int rc = check_bufs(who, {{"S", S, S_bytes, ((size_t)(nrows - 1) * ld + Skv) * 4, 4, false},
                                  {"P", P, P_bytes, (size_t)nrows * ld * 2, 2, false}}))
        return rc;
    HIP_TRY(launch_softmax_drop_rows(S, P, nrows, rows_per_bh, Skv, ld, scale, seed, layer, bh0, p_drop, (hipStream_t)stream));
    return DITTO_OK;
}
int ditto_bwd_softmax_rows(const float* S, size_t S_bytes, const float* dPd, size_t dPd_bytes, void* dS, size_t dS_bytes, int nrows,
                           int rows_per_bh, int Skv, int ld, float scale, uint64_t seed, int layer, int bh0, float p_drop,
                           ditto_stream_t stream) {
    const char* who = "ditto_bwd_softmax_rows";
    if (int rc = softmax_rows_shape(who, nrows, rows_per_bh, Skv, ld, scale, layer, bh0, p_drop)) return rc;
    const size_t in = ((size_t)(nrows - 1) * ld + Skv) * 4;
    if (int rc = check_bufs(who, {{"S", S, S_bytes, in, 4, false},
                                  {"dPd", dPd, dPd_bytes, in, 4, false},
                                  {"dS", dS, dS_bytes, (size_t)nrows * ld * 2, 2, false}}))
        return rc;
    HIP_TRY(launch_softmax_bwd_rows(S, dPd, dS, nrows, rows_per_bh, Skv, ld, scale, seed, layer, bh0, p_drop, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_bwd_small_linear(int mode, const float* x, size_t x_bytes, const float* W, size_t W_bytes, const float* dy, size_t dy_bytes,
                           float* out, size_t out_bytes, float* bias, size_t bias_bytes, int B, int I, int O, int silu_in,
                           ditto_stream_t stream) {
    const char* who = "ditto_bwd_small_linear";
    if (mode < DITTO_SMALL_LINEAR_FWD || mode > DITTO_SMALL_LINEAR_BWD_X || silu_in & ~1)
        return fail(DITTO_ERR_SHAPE, "%s: mode %d (0 fwd, 1 bwd_w, 2 bwd_x), silu_in %d (0 / 1)", who, mode, silu_in);
    if (B < 1 || I < 1 || O < 1 || B > 65535 || O > 65535 || I > (1 << 24))
        return fail(DITTO_ERR_SHAPE, "%s: B %d, I %d, O %d: need 1 <= B, O <= 65535, 1 <= I <= 2^24", who, B, I, O);
    const size_t xb = (size_t)B * I * 4, wb = (size_t)O * I * 4, yb = (size_t)B * O * 4, ob = (size_t)O * 4;
    const hipStream_t s = (hipStream_t)stream;
    if (mode == DITTO_SMALL_LINEAR_FWD) {
        if (dy) return fail(DITTO_ERR_ARG, "%s: the forward takes no dy", who);
        if (int rc = check_bufs(who, {{"x", x, x_bytes, xb, 4, false}, {"W", W, W_bytes, wb, 4, false},
                                      {"out", out, out_bytes, yb, 4, false}, {"bias", bias, bias_bytes, ob, 4, true}}))
            return rc;
        HIP_TRY(launch_small_linear_fwd(x, W, bias, out, B, I, O, silu_in != 0, s));
    } else if (mode == DITTO_SMALL_LINEAR_BWD_W) {
        if (W) return fail(DITTO_ERR_ARG, "%s: the weight gradient takes no W", who);
        if (int rc = check_bufs(who, {{"x", x, x_bytes, xb, 4, false}, {"dy", dy, dy_bytes, yb, 4, false},
                                      {"out", out, out_bytes, wb, 4, false}, {"bias", bias, bias_bytes, ob, 4, true}}))
            return rc;
        HIP_TRY(launch_small_linear_bwd_w(dy, x, out, bias, B, I, O, silu_in != 0, s));
    } else {
        if (bias) return fail(DITTO_ERR_ARG, "%s: the input gradient takes no bias", who);
        if (int rc = check_bufs(who, {{"x", x, x_bytes, xb, 4, !silu_in}, {"W", W, W_bytes, wb, 4, false},
                                      {"dy", dy, dy_bytes, yb, 4, false}, {"out", out, out_bytes, xb, 4, false}}))
            return rc;
        HIP_TRY(launch_small_linear_bwd_x(dy, W, x, out, B, I, O, silu_in != 0, s));
    }
    return DITTO_OK;
}

int ditto_bwd_embedding_scatter_add(const float* drows, size_t drows_bytes, const int64_t* ids, size_t ids_bytes, float* dtable,
                                    size_t dtable_bytes, int B, int V, int d, ditto_stream_t stream) {
    const char* who = "ditto_bwd_embedding_scatter_add";
    if (B < 1 || V < 1 || d < 1) return fail(DITTO_ERR_SHAPE, "%s: B %d, V %d, d %d must be positive", who, B, V, d);
    if (int rc = check_bufs(who, {{"drows", drows, drows_bytes, (size_t)B * d * 4, 4, false},
                                  {"ids", ids, ids_bytes, (size_t)B * 8, 8, false},
                                  {"dtable", dtable, dtable_bytes, (size_t)V * d * 4, 4, false}}))
        return rc;
    HIP_TRY(launch_embedding_scatter_add(drows, ids, dtable, B, V, d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_bwd_pack_bf16_t(const float* src, size_t src_bytes, void* dst, size_t dst_bytes, int rows, int cols, int ldT, int blk, int mult,
                          int row_off, ditto_stream_t stream) {
    const char* who = "ditto_bwd_pack_bf16_t";
    const long long last = last_packed_row(rows, blk, mult, row_off);
    if (last < 0 || cols < 1 || cols > 32 * 65535)
        return fail(DITTO_ERR_SHAPE, "%s: rows %d, cols %d, blk %d, mult %d, row_off %d: need rows, cols, blk, mult >= 1, row_off >= 0", who, rows,
                    cols, blk, mult, row_off);
    if (ldT <= last) return fail(DITTO_ERR_SHAPE, "%s: ldT %d does not cover the largest mapped row %lld", who, ldT, last);
    if (int rc = check_bufs(who, {{"src", src, src_bytes, (size_t)rows * cols * 4, 4, false},
                                  {"dst", dst, dst_bytes, ((size_t)(cols - 1) * ldT + (size_t)last + 1) * 2, 2, false}}))
        return rc;
    HIP_TRY(launch_pack_bf16_t(src, dst, rows, cols, ldT, blk, mult, row_off, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_bwd_unpack_rows(const float* src, size_t src_bytes, float* dst, size_t dst_bytes, int rows, int cols, int blk, int mult,
                          int row_off, ditto_stream_t stream) {
    const char* who = "ditto_bwd_unpack_rows";
    const long long last = last_packed_row(rows, blk, mult, row_off);
    if (last < 0 || cols < 4 || cols % 4)
        return fail(DITTO_ERR_SHAPE, "%s: rows %d, cols %d, blk %d, mult %d, row_off %d: need rows, blk, mult >= 1, row_off >= 0, cols %% 4 == 0",
                    who, rows, cols, blk, mult, row_off);
    if (int rc = check_bufs(who, {{"src", src, src_bytes, ((size_t)last + 1) * cols * 4, 16, false},
                                  {"dst", dst, dst_bytes, (size_t)rows * cols * 4, 16, false}}))
        return rc;
    HIP_TRY(launch_unpack_rows(src, dst, rows, cols, blk, mult, row_off, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_bwd_unpack_vec(const float* src, size_t src_bytes, float* dst, size_t dst_bytes, int rows, int blk, int mult, int row_off,
                         ditto_stream_t stream) {
    const char* who = "ditto_bwd_unpack_vec";
    const long long last = last_packed_row(rows, blk, mult, row_off);
    if (last < 0)
        return fail(DITTO_ERR_SHAPE, "%s: rows %d, blk %d, mult %d, row_off %d: need rows, blk, mult >= 1, row_off >= 0", who, rows, blk, mult,
                    row_off);
    if (int rc = check_bufs(who, {{"src", src, src_bytes, ((size_t)last + 1) * 4, 4, false},
                                  {"dst", dst, dst_bytes, (size_t)rows * 4, 4, false}}))
        return rc;
    HIP_TRY(launch_unpack_vec(src, dst, rows, blk, mult, row_off, (hipStream_t)stream));
    return DITTO_OK;
}

}  // extern "C"
