// guided_packed.hip — the fused update of one guided strided (DDIM) step over a PACKED batch (gfx950): guided_update.h's arithmetic
// with the utterances concatenated along the rows instead of padded.
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

// Packed batch: x2, eps2 [S, d] ([2S, d] under CFG: rows [0, S) conditional, [S, 2S) unconditional), utterance b owning rows
// [cu[b], cu[b+1]) of each half (guided_span's clamp).  The Philox quad index is the utterance-local one, ((row - cu[b]) d + col) / 4,
// so seeded packed sampling draws ditto_noise_normal's numbers.  No padding, hence no zeroing; a noise buffer is packed [S, d] like x.
template <int NOISE, bool CFG>
__global__ __launch_bounds__(256) void guided_update_packed_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                   const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                                   unsigned step, const float* __restrict__ w, const float* __restrict__ a,
                                                                   const float* __restrict__ ce, const float* __restrict__ cz,
                                                                   const int32_t* __restrict__ cu, int S, int d) {
    const int b = blockIdx.y;
    const GuidedSpan sp = guided_span(cu, b, S, d);
    const size_t half4 = (size_t)S * d / 4;
    const GuidedCoef k = guided_coef<NOISE, CFG>(a, ce, cz, w, seeds, b);
    guided_rows<NOISE, CFG, false>(reinterpret_cast<f32x4*>(x2) + sp.base4, reinterpret_cast<f32x4*>(x2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(noise) + sp.base4, k, step, true, sp.n4, sp.n4,
                                   blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

hipError_t launch_guided_update_packed(float* x2, const float* eps2, const float* noise, const int64_t* seeds, unsigned step,
                                       const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                       int B, int S, int max_N, int d, bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu) return hipErrorInvalidValue;
    return guided_dispatch(noise, seeds, cfg, [&](auto nz, auto cf) {
        hipLaunchKernelGGL((guided_update_packed_kernel<decltype(nz)::value, decltype(cf)::value>), guided_grid(max_N, d, B), dim3(256),
                           0, s, x2, eps2, noise, seeds, step, w, a, ce, cz, cu, S, d);
        return hipGetLastError();
    });
}

}  // namespace ditto
