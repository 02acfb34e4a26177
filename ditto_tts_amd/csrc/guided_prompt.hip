// guided_prompt.hip — the packed guided update with a SPEECH PROMPT per utterance (gfx950): the first prompt_len[b] rows of utterance b
// are clean latents that condition the rest (zero-shot voice cloning), so the update leaves them alone.  guided_update.h's arithmetic
// over the generated rows only; kernels of their own, so that guided_packed.hip and guided_tags.hip keep their machine code.
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

// guided_update_packed_kernel (TAGS false: the scalar `step`) or guided_update_packed_tags_kernel (TAGS true: tags[b], no draw at
// cz == 0) over the generated rows.  Every pointer is shifted past the prompt and the quad index runs from 0 at the first generated
// row: the Philox index is ((row - cu[b] - P_b) d + col) / 4, what an unprompted utterance of G_b rows draws, and P_b = 0 is the
// unprompted kernel bit for bit.  Prompt rows of x2 (both halves) and of eps2 are neither read nor written: 0 B per prompt element,
// 20 B per generated element under CFG.  prompt_len: device int32 [B], shared by the two halves.
template <int NOISE, bool CFG, bool TAGS>
__global__ __launch_bounds__(256) void guided_update_prompt_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                   const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                                   unsigned step, const unsigned* __restrict__ tags,
                                                                   const float* __restrict__ w, const float* __restrict__ a,
                                                                   const float* __restrict__ ce, const float* __restrict__ cz,
                                                                   const int32_t* __restrict__ cu, const int32_t* __restrict__ prompt_len,
                                                                   int S, int d) {
    const int b = blockIdx.y;
    const PromptSpan ps = prompt_span(cu, prompt_len, b, S, d);     // (guided_update.h)
    const GuidedSpan sp = {ps.base4 + ps.p4, ps.n4 - ps.p4};        // the generated rows [cu[b] + P_b, cu[b+1])
    const size_t half4 = (size_t)S * d / 4;
    const GuidedCoef k = guided_coef<NOISE, CFG>(a, ce, cz, w, seeds, b);
    const unsigned tag = TAGS ? (NOISE == 2 ? tags[b] : 0u) : step;
    guided_rows<NOISE, CFG, false>(reinterpret_cast<f32x4*>(x2) + sp.base4, reinterpret_cast<f32x4*>(x2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + sp.base4,
                                   reinterpret_cast<const f32x4*>(eps2) + half4 + sp.base4,
                                   reinterpret_cast<const f32x4*>(noise) + sp.base4, k, tag, TAGS ? k.cz != 0.f : true, sp.n4, sp.n4,
                                   blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

hipError_t launch_guided_update_prompt(float* x2, const float* eps2, const float* noise, const int64_t* seeds, unsigned step,
                                       const unsigned* tags, bool per_utt, const float* w, const float* a, const float* ce,
                                       const float* cz, const int32_t* cu, const int32_t* prompt_len, int B, int S, int max_N, int d,
                                       bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || !prompt_len || (per_utt && seeds && !tags))
        return hipErrorInvalidValue;
    return guided_dispatch(noise, seeds, cfg, [&](auto nz, auto cf) {
        if (per_utt)
            hipLaunchKernelGGL((guided_update_prompt_kernel<decltype(nz)::value, decltype(cf)::value, true>), guided_grid(max_N, d, B),
                               dim3(256), 0, s, x2, eps2, noise, seeds, 0u, tags, w, a, ce, cz, cu, prompt_len, S, d);
        else
            hipLaunchKernelGGL((guided_update_prompt_kernel<decltype(nz)::value, decltype(cf)::value, false>), guided_grid(max_N, d, B),
                               dim3(256), 0, s, x2, eps2, noise, seeds, step, tags, w, a, ce, cz, cu, prompt_len, S, d);
        return hipGetLastError();
    });
}

}  // namespace ditto
