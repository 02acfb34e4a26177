// guided.hip — the fused update of one guided strided (DDIM) step over a variable-length PADDED batch (gfx950); the row loop
// (update_rows with the DDIM line, its one PADDED user), the grid and the dispatch are guided_update.h's.
//
// One launch replaces the chain the strided sampler runs after each forward: two copies of x into the doubled batch,
// cfg_combine (which also allocates), the step's N(0,1) draw, linear_update and the zeroing of padded rows.
//   x2, eps2 fp32 [2B, N, d] under CFG ([conditional; unconditional], the forward's output over [text; null]), [B, N, d] without;
//   utterance b < B is written to x2[b] and, under CFG, to x2[B + b]: the next step's doubled input needs no copy.
//   Rows r >= speech_len[b]: 0 in both halves; x, eps2 and the noise are not read there and Philox does not run, so their contents
//   (NaN included) cannot matter.  speech_len NULL: every row is valid.
// A noise buffer is [B, N, d]; the Philox quad index is the padded layout's, which on every valid row is the utterance's own.
#include "guided_update.h"
#include "kernels.h"

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
    const GuidedCoef k = guided_coef<NOISE, CFG>(a, ce, cz, w, seeds, b);
    f32x4 *xc = reinterpret_cast<f32x4*>(x2) + (size_t)b * n4, *xu = reinterpret_cast<f32x4*>(x2) + (size_t)(B + b) * n4;
    const f32x4 *ec = reinterpret_cast<const f32x4*>(eps2) + (size_t)b * n4,
                *eu = reinterpret_cast<const f32x4*>(eps2) + (size_t)(B + b) * n4;
    const DdimLine<NOISE> ddim = {reinterpret_cast<const f32x4*>(noise) + (size_t)b * n4, k, step, true};
    update_rows<CFG ? EPS_CFG : EPS_COND, true>(xc, xu, ec, eu, ddim, nullptr, k.w, false, n4, valid4,
                                                blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

hipError_t launch_guided_update(float* x2, const float* eps2, const float* noise, const int64_t* seeds, unsigned step,
                                const float* w, const float* a, const float* ce, const float* cz, const int32_t* speech_len,
                                int B, int N, int d, bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || N <= 0 || B > 65535) return hipErrorInvalidValue;
    return guided_dispatch(noise, seeds, cfg, [&](auto nz, auto cf) {
        hipLaunchKernelGGL((guided_update_kernel<decltype(nz)::value, decltype(cf)::value>), guided_grid(N, d, B), dim3(256), 0, s, x2,
                           eps2, noise, seeds, step, w, a, ce, cz, speech_len, B, N, d);
        return hipGetLastError();
    });
}

}  // namespace ditto
