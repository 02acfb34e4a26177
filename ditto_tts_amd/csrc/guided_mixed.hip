// guided_mixed.hip — the packed guided update of a batch in which only SOME utterances are guided at this step (gfx950): guidance in a
// limited interval of noise levels (Kynkaanniemi et al. 2024) over a request stream, where every utterance stands at its own step
// of its own schedule.  The B utterances sit in rows [0, S) of x2 / eps2; the G guided ones have their unconditional copies compacted
// behind them in rows [S, S + S_G), copy g in rows [cu[B + g], cu[B + g + 1]) (cu = [cu_0 .. cu_B = S ; S + cu_G[1:]], B + G + 1
// offsets: what the forward over the B + G utterances reads).  partner[b]: the copy of utterance b, or -1.
//   with a partner:  e = fmaf(w, c - u, u), u read at the copy's rows; x' goes to b's rows and to the copy's   (the CFG instantiation)
//   without:         e = c; nothing of rows [S, S + S_G) is read or written                                     (the non-CFG one)
// guided_update.h's row loop (update_rows, EPS_CFG or EPS_COND, the DDIM line) over the generated rows, tags per utterance, no draw
// at cz == 0 (guided_packed.hip); a launch of its own for the layout and the branch on the partner.  HBM traffic per generated
// element: 20 B guided, 12 B (+ 4 B of a noise buffer) not; 0 B per prompt element.
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

// b = blockIdx.y is uniform over the workgroup: partner[b], the offsets and the coefficients come in through scalar loads and the
// branch on the partner is uniform.  Clamps: the partner into [-1, G - 1]; the copy's span has b's own length n_b, its first row
// clamped into [S, S + S_G - n_b] (no copy at all when n_b > S_G: the utterance is then updated without guidance).  The offset
// cu[B + g + 1] is not read: a bad table can make a copy's span run into the next copy's rows.  Wrong rows, never an access outside
// the S + S_G rows; b's own rows are always updated in full.  prompt_len NULL: no prompts.
template <int NOISE>
__global__ __launch_bounds__(256) void guided_update_mixed_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                  const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                                  const unsigned* __restrict__ tags, const float* __restrict__ w,
                                                                  const float* __restrict__ a, const float* __restrict__ ce,
                                                                  const float* __restrict__ cz, const int32_t* __restrict__ cu,
                                                                  const int32_t* __restrict__ partner,
                                                                  const int32_t* __restrict__ prompt_len, int B, int G, int S, int S_G,
                                                                  int d) {
    const int b = blockIdx.y;
    int r0 = cu[b];
    r0 = r0 < 0 ? 0 : (r0 > S - 1 ? S - 1 : r0);
    int n = cu[b + 1] - r0;
    n = n < 1 ? 1 : (n > S - r0 ? S - r0 : n);                      // utt_rows' clamp
    int g = partner[b];
    g = g < -1 ? -1 : (g > G - 1 ? G - 1 : g);
    int u0 = 0;
    if (n > S_G) g = -1;
    if (g >= 0) {
        u0 = cu[B + g];
        u0 = u0 < S ? S : (u0 > S + S_G - n ? S + S_G - n : u0);
    }
    int p = prompt_len ? prompt_len[b] : 0;
    p = p < 0 ? 0 : (p > n - 1 ? n - 1 : p);                        // window_span's clamp
    const size_t d4 = (size_t)d / 4, base4 = (size_t)(r0 + p) * d4, n4 = (size_t)(n - p) * d4;
    const GuidedCoef k = guided_coef<NOISE, true>(a, ce, cz, w, seeds, b);
    const unsigned tag = NOISE == 2 ? tags[b] : 0u;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + base4;
    const f32x4* nz = reinterpret_cast<const f32x4*>(noise) + base4;
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (g >= 0) {
        const size_t ub4 = (size_t)(u0 + p) * d4;
        update_rows<EPS_CFG, false>(xc, reinterpret_cast<f32x4*>(x2) + ub4, ec, reinterpret_cast<const f32x4*>(eps2) + ub4,
                                    DdimLine<NOISE>{nz, k, tag, k.cz != 0.f}, nullptr, k.w, false, n4, n4, i0, stride);
    } else {
        update_rows<EPS_COND, false>(xc, xc, ec, ec, DdimLine<NOISE>{nz, k, tag, k.cz != 0.f}, nullptr, k.w, false, n4, n4, i0, stride);
    }
}

hipError_t launch_guided_update_mixed(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const unsigned* tags,
                                      const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                      const int32_t* partner, const int32_t* prompt_len, int B, int G, int S, int S_G, int max_N, int d,
                                      hipStream_t s) {
    // (the conditions of check_mixed, ditto_api.hip, which both public entries pass through first)
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || !partner || !w || (seeds && !tags) ||
        !mixed_layout_ok(B, G, S, S_G))
        return hipErrorInvalidValue;
    const dim3 grid = guided_grid(max_N, d, B);
    noise_dispatch(noise, seeds, [&](auto nz) {
        hipLaunchKernelGGL((guided_update_mixed_kernel<decltype(nz)::value>), grid, dim3(256), 0, s, x2, eps2, noise, seeds, tags, w, a,
                           ce, cz, cu, partner, prompt_len, B, G, S, S_G, d);
    });
    return hipGetLastError();
}

}  // namespace ditto
