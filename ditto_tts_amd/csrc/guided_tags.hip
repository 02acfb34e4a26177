// guided_tags.hip — guided_packed.hip's fused update with one Philox step tag PER UTTERANCE (gfx950): what a batch whose utterances
// stand at different points of different schedules needs (continuous batching, ditto_tts_amd/serving.py).  A kernel of its own, not
// a mode of the scalar-tag one: skipping the draw at cz == 0 differs from that kernel in the sign of a zero.
#include "guided_update.h"
#include "kernels.h"

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
    const GuidedSpan sp = guided_span(cu, b, S, d);
    const size_t half4 = (size_t)S * d / 4;
    const GuidedCoef k = guided_coef<NOISE, CFG>(a, ce, cz, w, seeds, b);
    const unsigned step = NOISE == 2 ? tags[b] : 0u;
    guided_rows<NOISE, CFG, false>(reinterpret_cast<f32x4*>(x2) + sp.base4, reinterpret_cast<f32x4*>(x2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(noise) + sp.base4, k, step, k.cz != 0.f, sp.n4, sp.n4,
                                   blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

hipError_t launch_guided_update_packed_tags(float* x2, const float* eps2, const float* noise, const int64_t* seeds,
                                            const unsigned* tags, const float* w, const float* a, const float* ce, const float* cz,
                                            const int32_t* cu, int B, int S, int max_N, int d, bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || (seeds && !tags)) return hipErrorInvalidValue;
    return guided_dispatch(noise, seeds, cfg, [&](auto nz, auto cf) {
        hipLaunchKernelGGL((guided_update_packed_tags_kernel<decltype(nz)::value, decltype(cf)::value>), guided_grid(max_N, d, B),
                           dim3(256), 0, s, x2, eps2, noise, seeds, tags, w, a, ce, cz, cu, S, d);
        return hipGetLastError();
    });
}

}  // namespace ditto
