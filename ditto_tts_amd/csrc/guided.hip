// guided.hip — the fused update of one guided strided (DDIM) step over a variable-length batch (gfx950).
//
// One launch replaces the chain the strided sampler runs after each forward: two copies of x into the doubled batch,
// cfg_combine (which also allocates), the step's N(0,1) draw, linear_update and the zeroing of padded rows.
//   x2, eps2 fp32 [2B, N, d] under CFG ([conditional; unconditional], the forward's output over [text; null]), [B, N, d] without.
//   Utterance b < B, row r < speech_len[b], element e:
//     e' = CFG ? fmaf(w[b], c - u, u) : c          c = eps2[b], u = eps2[B + b]   (cfg_combine_kernel's expression)
//     x' = fmaf(a[b], x, fmaf(ce[b], e', cz[b] * z))                              (linear_update_kernel's; z = cz = 0 without noise)
//   written to x2[b] and, under CFG, to x2[B + b]: the next step's doubled input needs no copy.
//   Rows r >= speech_len[b]: 0 in both halves; x, eps2 and the noise are not read there and Philox does not run, so their contents
//   (NaN included) cannot matter.  speech_len NULL: every row is valid.
// Noise source (template): none, a buffer [B, N, d], or Philox from seeds[b] at `step` with the quad index of the padded layout —
// the bits of ditto_noise_normal(seeds, step) on every valid row (philox.h).
// Bytes per element of a valid row: CFG 4 reads (x, c, u, buffer noise) + 2 writes, without CFG 3 + 1; one read less without a
// noise buffer.  HBM-bound: judged against ~6.3 TB/s achievable.  16-byte lane accesses, grid (chunks, B) as linear_update's;
// d % 64 == 0, so a quad never straddles a row.
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace ditto {

template <int NOISE, bool CFG>   // NOISE: 0 none, 1 buffer, 2 Philox
__global__ __launch_bounds__(256) void guided_update_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                            const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                            unsigned step, const float* __restrict__ w, const float* __restrict__ a,
                                                            const float* __restrict__ ce, const float* __restrict__ cz,
                                                            const int32_t* __restrict__ speech_len, int B, int N, int d) {
    const int b = blockIdx.y;
    const size_t n4 = (size_t)N * d / 4;
    size_t valid4 = n4;
    if (speech_len) {
        const int v = speech_len[b], nb = v < 1 ? 1 : (v > N ? N : v);   // clamped into [1, N] as zero_rows_past_len's
        valid4 = (size_t)nb * d / 4;
    }
    const float ab = a[b], eb = ce[b], zb = NOISE ? cz[b] : 0.f, wb = CFG ? w[b] : 0.f;
    const unsigned long long seed = NOISE == 2 ? (unsigned long long)seeds[b] : 0ull;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + (size_t)b * n4;
    f32x4* xu = reinterpret_cast<f32x4*>(x2) + (size_t)(B + b) * n4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + (size_t)b * n4;
    const f32x4* eu = reinterpret_cast<const f32x4*>(eps2) + (size_t)(B + b) * n4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (i < valid4) {
            const f32x4 xv = xc[i];
            const f32x4 c = ec[i];
            f32x4 u = c;
            if (CFG) u = eu[i];
            f32x4 zv = {0.f, 0.f, 0.f, 0.f};
            if (NOISE == 1) zv = reinterpret_cast<const f32x4*>(noise)[(size_t)b * n4 + i];
            if (NOISE == 2) zv = normal4(seed, step, i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ev = CFG ? fmaf(wb, c[e] - u[e], u[e]) : c[e];
                o[e] = fmaf(ab, xv[e], fmaf(eb, ev, zb * zv[e]));
            }
        }
        xc[i] = o;
        if (CFG) xu[i] = o;
    }
}

template <int NOISE, bool CFG>
static hipError_t launch_guided(float* x2, const float* eps2, const float* noise, const int64_t* seeds, unsigned step,
                                const float* w, const float* a, const float* ce, const float* cz, const int32_t* speech_len,
                                int B, int N, int d, hipStream_t s) {
    const size_t n4 = (size_t)N * d / 4;
    size_t gx = (n4 + 255) / 256;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL((guided_update_kernel<NOISE, CFG>), dim3((unsigned)gx, B), dim3(256), 0, s, x2, eps2, noise, seeds, step, w,
                       a, ce, cz, speech_len, B, N, d);
    return hipGetLastError();
}

hipError_t launch_guided_update(float* x2, const float* eps2, const float* noise, const int64_t* seeds, unsigned step,
                                const float* w, const float* a, const float* ce, const float* cz, const int32_t* speech_len,
                                int B, int N, int d, bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || N <= 0 || B > 65535) return hipErrorInvalidValue;
    const int mode = seeds ? 2 : (noise ? 1 : 0);
#define DITTO_GUIDED(M)                                                                                                   \
    return cfg ? launch_guided<M, true>(x2, eps2, noise, seeds, step, w, a, ce, cz, speech_len, B, N, d, s)               \
               : launch_guided<M, false>(x2, eps2, noise, seeds, step, w, a, ce, cz, speech_len, B, N, d, s)
    if (mode == 2) DITTO_GUIDED(2);
    if (mode == 1) DITTO_GUIDED(1);
    DITTO_GUIDED(0);
#undef DITTO_GUIDED
}

}  // namespace ditto
