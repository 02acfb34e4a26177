// guided_refresh.hip — the packed guided update of a request stream whose utterances reuse the guidance direction between refresh
// steps (gfx950): guided_mixed.hip's layout and guided_reuse.hip's arithmetic in ONE launch.  Every utterance stands at its own step of
// its own refresh schedule (sampler.refresh_plan), so a step holds three kinds of utterance side by side; kind[b] says which:
//   1 refresh  dl = c - u, e = fmaf(w, dl, u), u read at the copy's rows; x' goes to b's rows and to the copy's, delta = dl on b's
//              generated rows: the bits of guided_update_mixed_kernel's partner branch.  Needs a usable partner, else it counts as 0
//   2 reuse    e = fmaf(w - 1.0f, delta, c): guided_update_reuse_kernel's LOAD line; delta is read and never written
//   0 plain    e = c; delta is neither read nor written                                      (values outside 0..2 count as 0)
// then x' = fmaf(a, x, fmaf(ce, e, cz z)) for every kind.  Reuse and plain touch nothing of rows [S, S + S_G).
// The B utterances sit in rows [0, S) of x2 / eps2 and the G refreshing ones have their unconditional copies compacted behind them in
// rows [S, S + S_G), as in guided_mixed.hip; delta fp32 [S, d] is row-aligned with rows [0, S).  guided_update.h's grid and span: grid
// (chunks, B), 256 threads, 16-byte lane accesses, b = blockIdx.y uniform over the workgroup, d % 64 == 0; tags per utterance, no
// Philox draw where cz[b] == 0; prompt rows of x2, eps2, delta and a noise buffer are neither read nor written.  The three kinds are
// update_rows' EPS_STORE, EPS_LOAD and EPS_COND with the DDIM line.  HBM traffic per generated element: refresh 24 B (x, c, u read; x',
// the copy and delta written), reuse 16 B (x, c, delta read; x' written), plain 12 B; + 4 B each with a noise buffer; 0 B per prompt
// element.
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

enum { KIND_PLAIN = 0, KIND_REFRESH = 1, KIND_REUSE = 2 };

// mixed_span's clamps (guided_update.h): b's generated rows lie inside [0, S) — so do delta's and the noise buffer's, which share
// their offset — and a copy's inside [S, S + S_G).  A bad cu / partner / kind / prompt_len gives wrong rows, never an access outside
// x2, eps2 [S + S_G, d] or delta [S, d].
template <int NOISE>
__global__ __launch_bounds__(256) void guided_update_refresh_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                    float* __restrict__ delta, const float* __restrict__ noise,
                                                                    const int64_t* __restrict__ seeds, const unsigned* __restrict__ tags,
                                                                    const float* __restrict__ w, const float* __restrict__ a,
                                                                    const float* __restrict__ ce, const float* __restrict__ cz,
                                                                    const int32_t* __restrict__ cu, const int32_t* __restrict__ partner,
                                                                    const int32_t* __restrict__ kind,
                                                                    const int32_t* __restrict__ prompt_len, int B, int G, int S, int S_G,
                                                                    int d) {
    const int b = blockIdx.y;
    const MixedSpan sp = mixed_span(cu, partner, prompt_len, b, B, G, S, S_G, d);
    int kd = kind[b];
    if (kd < KIND_PLAIN || kd > KIND_REUSE) kd = KIND_PLAIN;
    if (kd == KIND_REFRESH && sp.g < 0) kd = KIND_PLAIN;
    const GuidedCoef k = guided_coef<NOISE, true>(a, ce, cz, w, seeds, b);
    const unsigned tag = NOISE == 2 ? tags[b] : 0u;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + sp.base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + sp.base4;
    f32x4* dp = reinterpret_cast<f32x4*>(delta) + sp.base4;
    const DdimLine<NOISE> ddim = {reinterpret_cast<const f32x4*>(noise) + sp.base4, k, tag, k.cz != 0.f};
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (kd == KIND_REFRESH) {
        const size_t ub4 = (size_t)sp.urow * (size_t)(d / 4);
        update_rows<EPS_STORE, false>(xc, reinterpret_cast<f32x4*>(x2) + ub4, ec, reinterpret_cast<const f32x4*>(eps2) + ub4, ddim, dp,
                                      k.w, false, sp.n4, sp.n4, i0, stride);
    } else if (kd == KIND_REUSE) {
        update_rows<EPS_LOAD, false>(xc, xc, ec, ec, ddim, dp, k.w, false, sp.n4, sp.n4, i0, stride);
    } else {
        update_rows<EPS_COND, false>(xc, xc, ec, ec, ddim, dp, k.w, false, sp.n4, sp.n4, i0, stride);
    }
}

hipError_t launch_guided_update_refresh(float* x2, const float* eps2, float* delta, const float* noise, const int64_t* seeds,
                                        const unsigned* tags, const float* w, const float* a, const float* ce, const float* cz,
                                        const int32_t* cu, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len, int B,
                                        int G, int S, int S_G, int max_N, int d, hipStream_t s) {
    // (the conditions of check_refresh, ditto_api.hip, which both public entries pass through first)
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || !partner || !kind || !delta || !w || (seeds && !tags) ||
        !mixed_layout_ok(B, G, S, S_G))
        return hipErrorInvalidValue;
    const dim3 grid = guided_grid(max_N, d, B);
    noise_dispatch(noise, seeds, [&](auto nz) {
        hipLaunchKernelGGL((guided_update_refresh_kernel<decltype(nz)::value>), grid, dim3(256), 0, s, x2, eps2, delta, noise, seeds,
                           tags, w, a, ce, cz, cu, partner, kind, prompt_len, B, G, S, S_G, d);
    });
    return hipGetLastError();
}

}  // namespace ditto
