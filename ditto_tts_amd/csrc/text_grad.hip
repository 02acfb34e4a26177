// text_grad.hip — the text side of training for classifier-free guidance (include/ditto_text_grad.h): the three row kernels — the
// AdaLN text pool's backward over a packed batch, and condition dropout's select, forward and backward — and the two select entries.
// All three are bandwidth kernels: 16 bytes per lane, no LDS, no atomics, every output element written by exactly one thread, sums in
// a fixed order.  (The K/V path of the text gradient is a GEMM per layer, in ditto_train.hip's backward.)
#include "../../include/ditto_text_grad.h"
#include "common.h"
#include "kernels.h"
#include "model.h"

namespace ditto {
namespace {

DITTO_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the last utterance b of [0, B) with cu[b] <= r (b = 0 when there is none): packed_row_map_kernel's search (rowwise.hip)
DITTO_DEV int utt_of_row(const int32_t* __restrict__ cu, int B, int r) {
    int lo = 0, hi = B - 1;   // invariant: the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cu[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
inline unsigned quad_grid(size_t quads) {   // 256 threads per block, grid-stride beyond 2^20 blocks
    const size_t b = (quads + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > (1u << 20) ? (1u << 20) : b));
}

// d_text rows of utterance b += dpooled[b] / T_b.  Block (x, b): the rows [8x, 8x + 8) of the utterance; first row and length clamped
// as text_pool_packed_kernel (rowwise.hip packed_span) reads them, so the divisor is the forward's and no row leaves [0, S_T).
constexpr int POOL_ROWS = 8;
__global__ __launch_bounds__(256) void text_pool_bwd_packed_kernel(const float* __restrict__ dpooled, const int32_t* __restrict__ cu_t,
                                                                   float* __restrict__ d_text, int S_T, int max_T, int dt4) {
    const int b = blockIdx.y;
    const int lo = clampi(cu_t[b], 0, S_T - 1);
    const int n = cu_t[b + 1] - lo, cap = S_T - lo < max_T ? S_T - lo : max_T;
    const int Tb = n < 1 ? 1 : (n > cap ? cap : n);
    const int r0 = blockIdx.x * POOL_ROWS;
    if (r0 >= Tb) return;
    const int rows = Tb - r0 < POOL_ROWS ? Tb - r0 : POOL_ROWS;
    const float tb = (float)Tb;
    const f32x4* __restrict__ g = reinterpret_cast<const f32x4*>(dpooled) + (size_t)b * dt4;
    f32x4* __restrict__ out = reinterpret_cast<f32x4*>(d_text) + (size_t)(lo + r0) * dt4;
    for (int i = threadIdx.x; i < rows * dt4; i += 256) {
        const f32x4 v = g[i % dt4];
        f32x4 o = out[i];
        o[0] += v[0] / tb; o[1] += v[1] / tb; o[2] += v[2] / tb; o[3] += v[3] / tb;
        out[i] = o;
    }
}

// text_eff row r: a bit copy of its utterance's text row, or of the null row at the same position.  One 16-byte quad per thread and
// step; every index formed from the table is clamped into its buffer.
__global__ __launch_bounds__(256) void text_select_packed_kernel(const float* __restrict__ text, const float* __restrict__ null_rows,
                                                                 const int32_t* __restrict__ table, float* __restrict__ text_eff, int B,
                                                                 int S_T, int S_out, int T0, int dt4) {
    const int32_t *cu_out = table, *cu_text = table + B + 1, *drop = table + 2 * B + 2;
    const size_t n = (size_t)S_out * dt4, step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        const int r = (int)(i / dt4), c = (int)(i - (size_t)r * dt4);
        const int b = utt_of_row(cu_out, B, r), pos = r - cu_out[b];
        const f32x4* src = drop[b] ? reinterpret_cast<const f32x4*>(null_rows) + (size_t)clampi(pos, 0, T0 - 1) * dt4
                                   : reinterpret_cast<const f32x4*>(text) + (size_t)clampi(cu_text[b] + pos, 0, S_T - 1) * dt4;
        reinterpret_cast<f32x4*>(text_eff)[i] = src[c];
    }
}

// rows [0, S_T): d_text row r = its utterance's d_text_eff row, or zero when the utterance was dropped.  Rows [S_T, S_T + T0): d_null
// row r - S_T = the sum over the dropped utterances, in ascending b, of their d_text_eff row at that position — one accumulator per
// element, so the sum has one order.
__global__ __launch_bounds__(256) void text_select_packed_bwd_kernel(const float* __restrict__ d_text_eff, const int32_t* __restrict__ table,
                                                                     float* __restrict__ d_text, float* __restrict__ d_null, int B,
                                                                     int S_T, int S_out, int T0, int dt4) {
    const int32_t *cu_out = table, *cu_text = table + B + 1, *drop = table + 2 * B + 2;
    const f32x4* __restrict__ g = reinterpret_cast<const f32x4*>(d_text_eff);
    const size_t n_text = (size_t)S_T * dt4, n = n_text + (size_t)T0 * dt4, step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (i < n_text) {
            const int r = (int)(i / dt4), c = (int)(i - (size_t)r * dt4);
            const int b = utt_of_row(cu_text, B, r);
            if (!drop[b]) acc = g[(size_t)clampi(cu_out[b] + (r - cu_text[b]), 0, S_out - 1) * dt4 + c];
            reinterpret_cast<f32x4*>(d_text)[i] = acc;
        } else {
            const size_t j = i - n_text;
            const int r = (int)(j / dt4), c = (int)(j - (size_t)r * dt4);
            for (int b = 0; b < B; ++b) {
                if (!drop[b]) continue;
                const f32x4 v = g[(size_t)clampi(cu_out[b] + r, 0, S_out - 1) * dt4 + c];
                acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
            }
            reinterpret_cast<f32x4*>(d_null)[j] = acc;
        }
    }
}

// what both select entries refuse before they look at a pointer; the table is read on the host
int check_select(const char* who, const int32_t* table_host, size_t table_host_bytes, int B, int S_T, int S_out, int T0, int dt) {
    if (B < 1 || B > 65535 || S_T < B || S_out < B || T0 < 1 || dt < 4 || dt % 4 || dt > 65536 ||
        (unsigned long long)S_T * dt >= (1ull << 40) || (unsigned long long)S_out * dt >= (1ull << 40))
        return fail(DITTO_ERR_SHAPE, "%s: B %d, S_T %d, S_out %d, T0 %d, dt %d: need 1 <= B <= 65535, B <= S_T, B <= S_out, T0 >= 1, "
                    "dt %% 4 == 0, 4 <= dt <= 65536", who, B, S_T, S_out, T0, dt);
    if (!table_host) return fail(DITTO_ERR_ARG, "%s: null table_host", who);
    if (table_host_bytes < ((size_t)3 * B + 2) * 4)
        return fail(DITTO_ERR_SIZE, "%s: table_host too small: %zu < %zu bytes", who, table_host_bytes, ((size_t)3 * B + 2) * 4);
    const int32_t *cu_out = table_host, *cu_text = table_host + B + 1, *drop = table_host + 2 * B + 2;
    if (cu_out[0] != 0 || cu_text[0] != 0 || cu_out[B] != S_out || cu_text[B] != S_T)
        return fail(DITTO_ERR_SHAPE, "%s: the table's offsets must run from 0 to S_out = %d and from 0 to S_T = %d", who, S_out, S_T);
    for (int b = 0; b < B; ++b) {
        const long long lo = (long long)cu_out[b + 1] - cu_out[b], lt = (long long)cu_text[b + 1] - cu_text[b];
        if (drop[b] & ~1) return fail(DITTO_ERR_SHAPE, "%s: table: drop[%d] = %d is neither 0 nor 1", who, b, drop[b]);
        if (lo < 1 || lt < 1) return fail(DITTO_ERR_SHAPE, "%s: table: the offsets of utterance %d do not increase", who, b);
        if (lo != (drop[b] ? (long long)T0 : lt))
            return fail(DITTO_ERR_SHAPE, "%s: table: utterance %d (%s) has %lld rows in text_eff, %lld expected", who, b,
                        drop[b] ? "dropped" : "kept", lo, drop[b] ? (long long)T0 : lt);
    }
    return DITTO_OK;
}

}  // namespace

hipError_t launch_text_pool_bwd_packed(const float* dpooled, const int32_t* cu_t, float* d_text, int B, int S_T, int max_T, int dt,
                                       hipStream_t s) {
    if (!dpooled || !cu_t || !d_text || B < 1 || B > 65535 || S_T < 1 || max_T < 1 || dt < 4 || dt % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(text_pool_bwd_packed_kernel, dim3((max_T + POOL_ROWS - 1) / POOL_ROWS, B), dim3(256), 0, s, dpooled, cu_t, d_text,
                       S_T, max_T, dt / 4);
    return hipGetLastError();
}
hipError_t launch_text_select_packed(const float* text, const float* null_rows, const int32_t* table, float* text_eff, int B, int S_T,
                                     int S_out, int T0, int dt, hipStream_t s) {
    if (!text || !null_rows || !table || !text_eff || B < 1 || S_T < 1 || S_out < 1 || T0 < 1 || dt < 4 || dt % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(text_select_packed_kernel, dim3(quad_grid((size_t)S_out * (dt / 4))), dim3(256), 0, s, text, null_rows, table,
                       text_eff, B, S_T, S_out, T0, dt / 4);
    return hipGetLastError();
}
hipError_t launch_text_select_packed_bwd(const float* d_text_eff, const int32_t* table, float* d_text, float* d_null, int B, int S_T,
                                         int S_out, int T0, int dt, hipStream_t s) {
    if (!d_text_eff || !table || !d_text || !d_null || B < 1 || S_T < 1 || S_out < 1 || T0 < 1 || dt < 4 || dt % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(text_select_packed_bwd_kernel, dim3(quad_grid(((size_t)S_T + T0) * (dt / 4))), dim3(256), 0, s, d_text_eff, table,
                       d_text, d_null, B, S_T, S_out, T0, dt / 4);
    return hipGetLastError();
}

}  // namespace ditto

using namespace ditto;

extern "C" {

int ditto_text_select_packed(const float* text, size_t text_bytes, const float* null_rows, size_t null_rows_bytes,
                             const int32_t* table, size_t table_bytes, const int32_t* table_host, size_t table_host_bytes,
                             float* text_eff, size_t text_eff_bytes, int B, int S_T, int S_out, int T0, int dt,
                             ditto_stream_t stream) {
    const char* who = "ditto_text_select_packed";
    if (int rc = check_select(who, table_host, table_host_bytes, B, S_T, S_out, T0, dt)) return rc;
    if (int rc = check_bufs(who, {{"text", text, text_bytes, (size_t)S_T * dt * 4, 16, false},
                                  {"null_rows", null_rows, null_rows_bytes, (size_t)T0 * dt * 4, 16, false},
                                  {"table", table, table_bytes, ((size_t)3 * B + 2) * 4, 4, false},
                                  {"text_eff", text_eff, text_eff_bytes, (size_t)S_out * dt * 4, 16, false}}))
        return rc;
    HIP_TRY(launch_text_select_packed(text, null_rows, table, text_eff, B, S_T, S_out, T0, dt, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_text_select_packed_bwd(const float* d_text_eff, size_t d_text_eff_bytes, const int32_t* table, size_t table_bytes,
                                 const int32_t* table_host, size_t table_host_bytes, float* d_text, size_t d_text_bytes,
                                 float* d_null, size_t d_null_bytes, int B, int S_T, int S_out, int T0, int dt,
                                 ditto_stream_t stream) {
    const char* who = "ditto_text_select_packed_bwd";
    if (int rc = check_select(who, table_host, table_host_bytes, B, S_T, S_out, T0, dt)) return rc;
    if (int rc = check_bufs(who, {{"d_text_eff", d_text_eff, d_text_eff_bytes, (size_t)S_out * dt * 4, 16, false},
                                  {"table", table, table_bytes, ((size_t)3 * B + 2) * 4, 4, false},
                                  {"d_text", d_text, d_text_bytes, (size_t)S_T * dt * 4, 16, false},
                                  {"d_null", d_null, d_null_bytes, (size_t)T0 * dt * 4, 16, false}}))
        return rc;
    HIP_TRY(launch_text_select_packed_bwd(d_text_eff, table, d_text, d_null, B, S_T, S_out, T0, dt, (hipStream_t)stream));
    return DITTO_OK;
}

}  // extern "C"
