// guided_packed.hip — the fused update of one guided strided (DDIM) step over a PACKED batch (gfx950): guided_update.h's row loop
// (update_rows with the DDIM line) with the utterances concatenated along the rows instead of padded.  One kernel behind the six
// ditto_guided_update_packed* entries: a scalar step tag or one per utterance, over the whole utterance, the rows behind a speech prompt, or an infilling window.
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

// Packed batch: x2, eps2 [S, d] ([2S, d] under CFG: rows [0, S) conditional, [S, 2S) unconditional), utterance b owning rows
// [cu[b], cu[b+1]) of each half.  The update runs over window_span's window [cu[b] + P_b, cu[b+1] - Q_b) only (prompt_len, suffix_len:
// device int32 [B], shared by the two halves, either may be null): the clean context rows of x2 (both halves), of eps2 and of a noise
// buffer are neither read nor written, 0 B per context element, 20 B per generated element under CFG.  Every pointer is shifted to
// the window's first quad and the quad index runs from 0 there: the Philox index is ((row - cu[b] - P_b) d + col) / 4, what an
// utterance of G_b rows without context draws — ditto_noise_normal's numbers.  No padding, hence no zeroing; a noise buffer is packed
// [S, d] like x.
// TAGS false: every utterance draws at the scalar `step`.  TAGS true: utterance b at tags[b] (device uint32 [B]) — what a batch whose
// utterances stand at different points of different schedules needs (continuous batching, ditto_tts_amd/serving.py); an utterance
// whose cz is 0 (a sigma = 0 step of its schedule) draws nothing and adds cz * 0 = +0, the term of the no-noise instantiation, so it
// gets that instantiation's value; the test is uniform over the workgroup (b = blockIdx.y).
template <int NOISE, bool CFG, bool TAGS>
__global__ __launch_bounds__(256) void guided_update_packed_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                   const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                                   unsigned step, const unsigned* __restrict__ tags,
                                                                   const float* __restrict__ w, const float* __restrict__ a,
                                                                   const float* __restrict__ ce, const float* __restrict__ cz,
                                                                   const int32_t* __restrict__ cu, const int32_t* __restrict__ prompt_len,
                                                                   const int32_t* __restrict__ suffix_len, int S, int d) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);     // (guided_update.h)
    const size_t base4 = ws.base4 + ws.p4, half4 = (size_t)S * d / 4;
    const GuidedCoef k = guided_coef<NOISE, CFG>(a, ce, cz, w, seeds, b);
    const unsigned tag = TAGS ? (NOISE == 2 ? tags[b] : 0u) : step;
    f32x4 *xc = reinterpret_cast<f32x4*>(x2) + base4, *xu = reinterpret_cast<f32x4*>(x2) + half4 + base4;
    const f32x4 *ec = reinterpret_cast<const f32x4*>(eps2) + base4, *eu = reinterpret_cast<const f32x4*>(eps2) + half4 + base4;
    const DdimLine<NOISE> ddim = {reinterpret_cast<const f32x4*>(noise) + base4, k, tag, TAGS ? k.cz != 0.f : true};
    update_rows<CFG ? EPS_CFG : EPS_COND, false>(xc, xu, ec, eu, ddim, nullptr, k.w, false, ws.g4, ws.g4,
                                                 blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

hipError_t launch_guided_update_packed(float* x2, const float* eps2, const float* noise, const int64_t* seeds, unsigned step,
                                       const unsigned* tags, bool per_utt, const float* w, const float* a, const float* ce,
                                       const float* cz, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                       int S, int max_N, int d, bool cfg, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || (per_utt && seeds && !tags)) return hipErrorInvalidValue;
    return guided_dispatch(noise, seeds, cfg, [&](auto nz, auto cf) {
        auto go = [&](auto tg) {
            hipLaunchKernelGGL((guided_update_packed_kernel<decltype(nz)::value, decltype(cf)::value, decltype(tg)::value>),
                               guided_grid(max_N, d, B), dim3(256), 0, s, x2, eps2, noise, seeds, per_utt ? 0u : step, tags, w, a, ce, cz,
                               cu, prompt_len, suffix_len, S, d);
        };
        per_utt ? go(std::true_type{}) : go(std::false_type{});
        return hipGetLastError();
    });
}

}  // namespace ditto
