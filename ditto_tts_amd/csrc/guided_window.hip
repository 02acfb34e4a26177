// guided_window.hip — the packed guided updates over a WINDOW per utterance (gfx950): speech infilling.  The first prompt_len[b] and
// the last suffix_len[b] rows of utterance b are clean latents that condition the rows in between, so the update leaves both alone.
// guided_update.h's arithmetic (and guided_multistep.hip's, restated) over the window [cu[b] + P_b, cu[b+1] - Q_b) only; kernels of
// their own, so that guided_packed.hip, guided_tags.hip, guided_prompt.hip and guided_multistep.hip keep their machine code.
#include "ditto_hip.h"
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

// guided_update_prompt_kernel with a second boundary.  Every pointer is shifted to the window's first quad and the quad index runs
// from 0 there: the Philox index is ((row - cu[b] - P_b) d + col) / 4, what an unprompted utterance of G_b rows draws, and Q_b = 0 is
// the prompt kernel bit for bit.  Context rows of x2 (both halves), of eps2 and of a noise buffer are neither read nor written, on
// either side: 0 B per context element, 20 B per generated element under CFG.  prompt_len (may be null: P = 0), suffix_len: device
// int32 [B], shared by the two halves.
template <int NOISE, bool CFG, bool TAGS>
__global__ __launch_bounds__(256) void guided_update_window_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                   const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                                   unsigned step, const unsigned* __restrict__ tags,
                                                                   const float* __restrict__ w, const float* __restrict__ a,
                                                                   const float* __restrict__ ce, const float* __restrict__ cz,
                                                                   const int32_t* __restrict__ cu, const int32_t* __restrict__ prompt_len,
                                                                   const int32_t* __restrict__ suffix_len, int S, int d) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);     // (guided_update.h)
    const GuidedSpan sp = {ws.base4 + ws.p4, ws.g4};                            // the window [cu[b] + P_b, cu[b+1] - Q_b)
    const size_t half4 = (size_t)S * d / 4;
    const GuidedCoef k = guided_coef<NOISE, CFG>(a, ce, cz, w, seeds, b);
    const unsigned tag = TAGS ? (NOISE == 2 ? tags[b] : 0u) : step;
    guided_rows<NOISE, CFG, false>(reinterpret_cast<f32x4*>(x2) + sp.base4, reinterpret_cast<f32x4*>(x2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(noise) + sp.base4, k, tag, TAGS ? k.cz != 0.f : true, sp.n4, sp.n4,
                                   blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

hipError_t launch_guided_update_window(float* x2, const float* eps2, const float* noise, const int64_t* seeds, unsigned step,
                                       const unsigned* tags, bool per_utt, const float* w, const float* a, const float* ce,
                                       const float* cz, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                       int S, int max_N, int d, bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || !suffix_len || (per_utt && seeds && !tags))
        return hipErrorInvalidValue;
    return guided_dispatch(noise, seeds, cfg, [&](auto nz, auto cf) {
        if (per_utt)
            hipLaunchKernelGGL((guided_update_window_kernel<decltype(nz)::value, decltype(cf)::value, true>), guided_grid(max_N, d, B),
                               dim3(256), 0, s, x2, eps2, noise, seeds, 0u, tags, w, a, ce, cz, cu, prompt_len, suffix_len, S, d);
        else
            hipLaunchKernelGGL((guided_update_window_kernel<decltype(nz)::value, decltype(cf)::value, false>), guided_grid(max_N, d, B),
                               dim3(256), 0, s, x2, eps2, noise, seeds, step, tags, w, a, ce, cz, cu, prompt_len, suffix_len, S, d);
        return hipGetLastError();
    });
}

// guided_multistep.hip's multistep_rows, restated (that file keeps its machine code): quads [i0, n4) of one utterance's window at a
// grid stride.  PREV false: q is written and never read
template <bool CFG, bool PREV>
__device__ __forceinline__ void multistep_window_rows(f32x4* xc, f32x4* xu, const f32x4* ec, const f32x4* eu, f32x4* qp,
                                                      const ditto_multistep_coef& k, size_t n4, size_t i0, size_t stride) {
    for (size_t i = i0; i < n4; i += stride) {
        const f32x4 xv = xc[i];
        const f32x4 c = ec[i];
        f32x4 u = c;
        if (CFG) u = eu[i];
        f32x4 qv = {0.f, 0.f, 0.f, 0.f};
        if (PREV) qv = qp[i];
        f32x4 o, p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ev = CFG ? fmaf(k.w, c[e] - u[e], u[e]) : c[e];
            p[e] = fmaf(k.kx, xv[e], k.ke * ev);
            o[e] = fmaf(k.a, xv[e], fmaf(k.b, p[e], PREV ? k.g * qv[e] : 0.f));
        }
        xc[i] = o;
        if (CFG) xu[i] = o;
        qp[i] = p;
    }
}

// multistep_update_kernel over the window: the context rows of x2, eps2 and q are neither read nor written, on either side
template <bool CFG, bool PER_UTT>
__global__ __launch_bounds__(256) void multistep_update_window_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                      float* __restrict__ q, ditto_multistep_coef step,
                                                                      const ditto_multistep_coef* __restrict__ coefs,
                                                                      const float* __restrict__ w, const int32_t* __restrict__ cu,
                                                                      const int32_t* __restrict__ prompt_len,
                                                                      const int32_t* __restrict__ suffix_len, int S, int d) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);
    const GuidedSpan sp = {ws.base4 + ws.p4, ws.g4};
    ditto_multistep_coef k = step;
    if (PER_UTT) k = coefs[b];
    else k.w = CFG ? w[b] : 0.f;
    const size_t half4 = (size_t)S * d / 4;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + sp.base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + sp.base4;
    f32x4* qp = reinterpret_cast<f32x4*>(q) + sp.base4;
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (k.use_prev)
        multistep_window_rows<CFG, true>(xc, xc + half4, ec, ec + half4, qp, k, sp.n4, i0, stride);
    else
        multistep_window_rows<CFG, false>(xc, xc + half4, ec, ec + half4, qp, k, sp.n4, i0, stride);
}

hipError_t launch_multistep_update_window(float* x2, const float* eps2, float* q, const ditto_multistep_coef* step,
                                          const ditto_multistep_coef* coefs, const float* w, const int32_t* cu,
                                          const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, bool cfg,
                                          hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || !suffix_len || !q || !step == !coefs || (step && cfg && !w))
        return hipErrorInvalidValue;
    const dim3 grid = guided_grid(max_N, d, B);
    const ditto_multistep_coef none = {};
    auto go = [&](auto cf, auto pu) {
        hipLaunchKernelGGL((multistep_update_window_kernel<decltype(cf)::value, decltype(pu)::value>), grid, dim3(256), 0, s, x2, eps2,
                           q, step ? *step : none, coefs, w, cu, prompt_len, suffix_len, S, d);
    };
    if (cfg) coefs ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
    else coefs ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
    return hipGetLastError();
}

}  // namespace ditto
