// guided_tags.hip — guided_packed.hip's fused update with one Philox step tag PER UTTERANCE (gfx950): what a batch whose utterances
// stand at different points of different schedules needs (continuous batching, ditto_tts_amd/serving.py).  Its own translation unit,
// so that the instantiations of guided.hip and guided_packed.hip stay as they were.
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace ditto {

// guided_update_packed_kernel with `tags[b]` in the place of the scalar `step`: utterance b gets the bits that kernel gives it at
// step = tags[b].  An utterance whose cz is 0 (a sigma = 0 step of its schedule) draws nothing and adds cz * 0 = +0, the term of the
// no-noise instantiation, so it gets that instantiation's value; the test is uniform over the workgroup (b = blockIdx.y).
// HBM traffic as the scalar-tag kernel: 20 B per element of a valid row under CFG (x, eps_c, eps_u read; both halves written).
template <int NOISE, bool CFG>
__global__ __launch_bounds__(256) void guided_update_packed_tags_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                        const float* __restrict__ noise,
                                                                        const int64_t* __restrict__ seeds,
                                                                        const unsigned* __restrict__ tags, const float* __restrict__ w,
                                                                        const float* __restrict__ a, const float* __restrict__ ce,
                                                                        const float* __restrict__ cz, const int32_t* __restrict__ cu,
                                                                        int S, int d) {
    const int b = blockIdx.y;
    int r0 = cu[b];
    r0 = r0 < 0 ? 0 : (r0 > S - 1 ? S - 1 : r0);
    const int n = cu[b + 1] - r0, nb = n < 1 ? 1 : (n > S - r0 ? S - r0 : n);
    const size_t half4 = (size_t)S * d / 4, base4 = (size_t)r0 * d / 4, n4 = (size_t)nb * d / 4;
    const float ab = a[b], eb = ce[b], zb = NOISE ? cz[b] : 0.f, wb = CFG ? w[b] : 0.f;
    const unsigned long long seed = NOISE == 2 ? (unsigned long long)seeds[b] : 0ull;
    const unsigned step = NOISE == 2 ? tags[b] : 0u;
    const bool draw = NOISE == 2 && zb != 0.f;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + base4;
    f32x4* xu = reinterpret_cast<f32x4*>(x2) + half4 + base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + base4;
    const f32x4* eu = reinterpret_cast<const f32x4*>(eps2) + half4 + base4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 xv = xc[i];
        const f32x4 c = ec[i];
        f32x4 u = c;
        if (CFG) u = eu[i];
        f32x4 zv = {0.f, 0.f, 0.f, 0.f};
        if (NOISE == 1) zv = reinterpret_cast<const f32x4*>(noise)[base4 + i];
        if (draw) zv = normal4(seed, step, i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ev = CFG ? fmaf(wb, c[e] - u[e], u[e]) : c[e];
            o[e] = fmaf(ab, xv[e], fmaf(eb, ev, zb * zv[e]));
        }
        xc[i] = o;
        if (CFG) xu[i] = o;
    }
}

template <int NOISE, bool CFG>
static hipError_t launch_guided_tags(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const unsigned* tags,
                                     const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu, int B, int S,
                                     int max_N, int d, hipStream_t s) {
    const size_t n4 = (size_t)max_N * d / 4;
    size_t gx = (n4 + 255) / 256;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL((guided_update_packed_tags_kernel<NOISE, CFG>), dim3((unsigned)gx, B), dim3(256), 0, s, x2, eps2, noise, seeds,
                       tags, w, a, ce, cz, cu, S, d);
    return hipGetLastError();
}

hipError_t launch_guided_update_packed_tags(float* x2, const float* eps2, const float* noise, const int64_t* seeds,
                                            const unsigned* tags, const float* w, const float* a, const float* ce, const float* cz,
                                            const int32_t* cu, int B, int S, int max_N, int d, bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || (seeds && !tags)) return hipErrorInvalidValue;
    const int mode = seeds ? 2 : (noise ? 1 : 0);
#define DITTO_GUIDED(M)                                                                                                        \
    return cfg ? launch_guided_tags<M, true>(x2, eps2, noise, seeds, tags, w, a, ce, cz, cu, B, S, max_N, d, s)                \
               : launch_guided_tags<M, false>(x2, eps2, noise, seeds, tags, w, a, ce, cz, cu, B, S, max_N, d, s)
    if (mode == 2) DITTO_GUIDED(2);
    if (mode == 1) DITTO_GUIDED(1);
    DITTO_GUIDED(0);
#undef DITTO_GUIDED
}

}  // namespace ditto
