// train_packed.hip — the one backward row kernel that needs the packed layout: the GlobalAdaLN reductions per utterance (reference
// src/components/DiT.py:25-40 under autograd: h0 = xhat (1 + s_t + s_x) + (b_t + b_x), so the gradient of utterance b's (scale, shift)
// vectors is [sum dh * xhat | sum dh] over ITS rows [cu[b], cu[b+1]) of the packed [S, d] stream).  train.hip's ln_bwd_kernel reduces
// over groups of a fixed rows_per_group; here a workgroup's rows come from the offsets, so a partial never straddles an utterance, and
// the second stage sums an utterance's partials in chunk order: no atomics, the same bits every time.
#include "gemm_common.h"

namespace ditto {

namespace {

// one wave per row; workgroup (chunk, b) owns rows [chunk * rpc, (chunk + 1) * rpc) of utterance b and writes its partial
// [sum dy * xhat | sum dy] row to partial[(b * chunks + chunk)][2d] (zeros when the utterance ends before the chunk)
template <int CH>
__global__ __launch_bounds__(256) void adaln_bwd_packed_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const int32_t* __restrict__ cu, int S, int max_len,
                                                               float* __restrict__ partial, int d, int rpc, int chunks) {
    __shared__ f32x4 red[4][2 * CH * 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int nv = d >> 2;
    // the utterance's first row clamped into [0, S - 1], its length into [1, min(max_len, S - first)]: a bad offset cannot address
    // outside the buffers
    int lo = cu[b];
    lo = lo < 0 ? 0 : (lo > S - 1 ? S - 1 : lo);
    int len = cu[b + 1] - lo;
    const int cap = S - lo < max_len ? S - lo : max_len;
    len = len < 1 ? 1 : (len > cap ? cap : len);
    const int rbeg = chunk * rpc;
    const int rend = rbeg + rpc < len ? rbeg + rpc : len;
    f32x4 dg[CH], db[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        dg[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        db[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int r = rbeg + wv; r < rend; r += 4) {
        const size_t row = (size_t)lo + r;
        const f32x4* xr = reinterpret_cast<const f32x4*>(x + row * d);
        const f32x4* dr = reinterpret_cast<const f32x4*>(dy + row * d);
        f32x4 v[CH], gy[CH];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = lane + 64 * c;
            if (i < nv) {
                v[c] = xr[i];
                gy[c] = dr[i];
                s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
            } else {
                v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
                gy[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        const float mean = wave_sum(s) / (float)d;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = lane + 64 * c;
            if (i < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dl = v[c][e] - mean;
                    q += dl * dl;
                }
            }
        }
        const float rstd = rsqrtf(wave_sum(q) / (float)d + 1e-5f);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = lane + 64 * c;
            if (i < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dg[c][e] += gy[c][e] * ((v[c][e] - mean) * rstd);
                    db[c][e] += gy[c][e];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        red[wv][c * 64 + lane] = dg[c];
        red[wv][(CH + c) * 64 + lane] = db[c];
    }
    __syncthreads();
    float* prow = partial + ((size_t)b * chunks + chunk) * 2 * d;
    for (int idx = threadIdx.x; idx < 2 * CH * 64; idx += 256) {
        const int c = (idx / 64) % CH, half = idx / (64 * CH), i = (idx & 63) + 64 * c;
        if (i < nv) {
            const f32x4 r = (red[0][idx] + red[1][idx]) + (red[2][idx] + red[3][idx]);
            *reinterpret_cast<f32x4*>(prow + (size_t)half * d + 4 * i) = r;
        }
    }
}

// out[b][j] = sum over chunks, in chunk order, of partial[(b * chunks + c)][j]
__global__ __launch_bounds__(256) void segment_partials_kernel(const float* __restrict__ partial, int chunks, int n,
                                                               float* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= n) return;
    const float* p = partial + (size_t)b * chunks * n + j;
    float a = 0.f;
    for (int c = 0; c < chunks; ++c) a += p[(size_t)c * n];
    out[(size_t)b * n + j] = a;
}

inline int adaln_bwd_packed_chunks(int max_len, int B) {
    int chunks = (1024 + B - 1) / B;
    const int maxc = (max_len + 15) / 16;
    if (chunks > maxc) chunks = maxc;
    return chunks < 1 ? 1 : chunks;
}

}  // namespace

size_t adaln_bwd_packed_scratch_bytes(int max_len, int B, int d) {
    return (size_t)B * adaln_bwd_packed_chunks(max_len, B) * 2 * d * 4;
}

// dmod fp32 [B, 2d] = [sum dy * xhat | sum dy] over utterance b's rows of dy, x [S, d]; cu device int32 [B + 1]; max_len: the longest
// utterance (host-validated; sizes the grid).  scratch: adaln_bwd_packed_scratch_bytes(max_len, B, d)
hipError_t launch_adaln_bwd_packed(const float* dy, const float* x, const int32_t* cu, int B, int S, int max_len, int d, float* dmod,
                                   float* scratch, hipStream_t s) {
    if (d % 4 || d > 2048 || B <= 0 || S <= 0 || max_len <= 0 || B > 65535 || !cu || !scratch) return hipErrorInvalidValue;
    const int ch = (d / 4 + 63) / 64;
    const int chunks = adaln_bwd_packed_chunks(max_len, B);
    const int rpc = (max_len + chunks - 1) / chunks;
    dim3 grid(chunks, B), block(256);
#define ALB_CASE(C)                                                                                                          \
    case C:                                                                                                                  \
        hipLaunchKernelGGL((adaln_bwd_packed_kernel<C>), grid, block, 0, s, dy, x, cu, S, max_len, scratch, d, rpc, chunks); \
        break;
    switch (ch) {
        ALB_CASE(1) ALB_CASE(2) ALB_CASE(3) ALB_CASE(4) ALB_CASE(5) ALB_CASE(6) ALB_CASE(7) ALB_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef ALB_CASE
    hipLaunchKernelGGL(segment_partials_kernel, dim3((2 * d + 255) / 256, B), dim3(256), 0, s, scratch, chunks, 2 * d, dmod);
    return hipGetLastError();
}

}  // namespace ditto
