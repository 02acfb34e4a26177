// guided_reuse.hip — the packed guided updates that keep and reuse the guidance direction (gfx950): the unconditional forward runs
// only at every k-th guided step (the "CFG cache" of FasterCache, Lv et al. 2024, without its frequency reweighting), and the steps in
// between add the last direction delta = c - u to the conditional prediction of the moment:
//   u + w (c - u) = c + (w - 1)(c - u)  ~  c_now + (w - 1) delta_last
// delta fp32 [S, d] is row-aligned with the conditional half.  Over guided_update.h's span and grid, like guided_packed.hip and
// guided_multistep.hip: grid (chunks, B), 256 threads, 16-byte lane accesses, b = blockIdx.y uniform over the workgroup, d % 64 == 0;
// the context rows of x2, eps, delta, q and a noise buffer are neither read nor written.
//   STORE (a refresh step; eps [2S, d]):   dl = c - u,  e = fmaf(w, dl, u),  delta = dl       update_rows' EPS_STORE, which is EPS_CFG
//                                          with dl kept: x' (and q) have the CFG kernels' bits, written to both halves
//   LOAD  (a reuse step;  eps [S, d]):     e = fmaf(w - 1, delta, c)                          EPS_LOAD: delta is read and never written; x' goes
//                                          to the conditional half and, with the run-time `mirror`, to the row + S of the other
// then guided_update.h's DDIM line x' = fmaf(a, x, fmaf(ce, e, cz z)) with the scalar-tag noise (every utterance draws, window-local
// Philox index), or its multistep lines.  The multistep kernel runs update_rows; the DDIM kernel keeps the same loop written out, for
// the reason given above it.  HBM-bound, per generated element: STORE the CFG update's bytes + 4 (20 + 4 DDIM
// without a noise buffer, 28 + 4 multistep with history); LOAD x, c and delta read (12 B) and x' written (4 B), 4 B more than the unguided
// update, + 4 B noise buffer, + 4 B mirror, + 8 B multistep history (q read and written).
#include "ditto_hip.h"
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

enum { REUSE_STORE = 1, REUSE_LOAD = 2 };                                      // the entries' `mode`
template <int MODE> constexpr int reuse_eps_mode = MODE == REUSE_STORE ? EPS_STORE : EPS_LOAD;

// The one kernel that keeps a row loop of its own: update_rows<EPS_STORE / EPS_LOAD> with the DDIM line, written out as it stood
// before the other loops were folded.  Routed through update_rows its six instantiations compile to the same optimised IR, but the
// return block of an inlined loop lands behind the loop where a loop written in the __global__ function has it in front, and the
// code that follows differs: the Philox LOAD kernel came out at 294 instructions for 287 and 34 VGPRs for 32, and measured 0.4 %
// and 0.5 % slower than its parent in two runs beside an A/A spread of +-0.25 % (the five others stayed inside theirs; every digest
// was equal).  tests/test_gpu_reuse_update.py and tests/test_gpu_refresh_update.py hold this text to update_rows' bits.
template <int NOISE, int MODE>
__global__ __launch_bounds__(256) void guided_update_reuse_kernel(float* __restrict__ x2, const float* __restrict__ eps,
                                                                  float* __restrict__ delta, const float* __restrict__ noise,
                                                                  const int64_t* __restrict__ seeds, unsigned step,
                                                                  const float* __restrict__ w, const float* __restrict__ a,
                                                                  const float* __restrict__ ce, const float* __restrict__ cz,
                                                                  const int32_t* __restrict__ cu, const int32_t* __restrict__ prompt_len,
                                                                  const int32_t* __restrict__ suffix_len, int S, int d, int mirror) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);     // (guided_update.h)
    const size_t base4 = ws.base4 + ws.p4, half4 = (size_t)S * d / 4;
    const GuidedCoef k = guided_coef<NOISE, true>(a, ce, cz, w, seeds, b);
    const float wm1 = k.w - 1.0f;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + base4;
    f32x4* xu = xc + half4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps) + base4;
    const f32x4* eu = ec + half4;                                              // STORE only: eps is [2S, d] there
    f32x4* dp = reinterpret_cast<f32x4*>(delta) + base4;
    const f32x4* nz = reinterpret_cast<const f32x4*>(noise) + base4;
    const bool both = MODE == REUSE_STORE || mirror != 0;                       // uniform: a scalar branch
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < ws.g4; i += stride) {
        const f32x4 xv = xc[i];
        const f32x4 c = ec[i];
        f32x4 u = c, dl;
        if (MODE == REUSE_STORE) u = eu[i];
        else dl = dp[i];
        f32x4 zv = {0.f, 0.f, 0.f, 0.f};
        if (NOISE == 1) zv = nz[i];
        if (NOISE == 2) zv = normal4(k.seed, step, i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dv = MODE == REUSE_STORE ? c[e] - u[e] : dl[e];
            const float ev = MODE == REUSE_STORE ? fmaf(k.w, dv, u[e]) : fmaf(wm1, dv, c[e]);
            dl[e] = dv;
            o[e] = fmaf(k.a, xv[e], fmaf(k.ce, ev, k.cz * zv[e]));
        }
        xc[i] = o;
        if (both) xu[i] = o;
        if (MODE == REUSE_STORE) dp[i] = dl;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void multistep_update_reuse_kernel(float* __restrict__ x2, const float* __restrict__ eps,
                                                                     float* __restrict__ q, float* __restrict__ delta,
                                                                     ditto_multistep_coef step, const float* __restrict__ w,
                                                                     const int32_t* __restrict__ cu, const int32_t* __restrict__ prompt_len,
                                                                     const int32_t* __restrict__ suffix_len, int S, int d, int mirror) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);     // (guided_update.h)
    const size_t base4 = ws.base4 + ws.p4, half4 = (size_t)S * d / 4;
    ditto_multistep_coef k = step;
    k.w = w[b];
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps) + base4;
    f32x4* qp = reinterpret_cast<f32x4*>(q) + base4;
    f32x4* dp = reinterpret_cast<f32x4*>(delta) + base4;
    const bool both = mirror != 0;                                              // LOAD only; uniform: a scalar branch
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    constexpr int EPS = reuse_eps_mode<MODE>;
    if (k.use_prev)
        update_rows<EPS, false>(xc, xc + half4, ec, ec + half4, MultistepLine<true>{qp, k}, dp, k.w, both, ws.g4, ws.g4, i0, stride);
    else
        update_rows<EPS, false>(xc, xc + half4, ec, ec + half4, MultistepLine<false>{qp, k}, dp, k.w, both, ws.g4, ws.g4, i0, stride);
}

static bool reuse_args_ok(const void* x2, const void* eps, const void* delta, const float* w, const int32_t* cu, int B, int S, int max_N,
                          int d, int mode, int mirror) {
    return x2 && eps && delta && w && cu && d > 0 && d % 64 == 0 && B > 0 && S > 0 && max_N > 0 && B <= 65535 &&
           (mode == REUSE_STORE || mode == REUSE_LOAD) && !(mode == REUSE_STORE && mirror);
}

hipError_t launch_guided_update_reuse(float* x2, const float* eps, float* delta, const float* noise, const int64_t* seeds, unsigned step,
                                      const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                      const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, int mode,
                                      int mirror, hipStream_t s) {
    if (!reuse_args_ok(x2, eps, delta, w, cu, B, S, max_N, d, mode, mirror) || (noise && seeds)) return hipErrorInvalidValue;
    auto go = [&](auto nz, auto md) {
        hipLaunchKernelGGL((guided_update_reuse_kernel<decltype(nz)::value, decltype(md)::value>), guided_grid(max_N, d, B), dim3(256), 0,
                           s, x2, eps, delta, noise, seeds, step, w, a, ce, cz, cu, prompt_len, suffix_len, S, d, mirror);
    };
    noise_dispatch(noise, seeds, [&](auto nz) {
        mode == REUSE_STORE ? go(nz, std::integral_constant<int, REUSE_STORE>{}) : go(nz, std::integral_constant<int, REUSE_LOAD>{});
    });
    return hipGetLastError();
}

hipError_t launch_multistep_update_reuse(float* x2, const float* eps, float* q, float* delta, const ditto_multistep_coef* step,
                                         const float* w, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                         int S, int max_N, int d, int mode, int mirror, hipStream_t s) {
    if (!reuse_args_ok(x2, eps, delta, w, cu, B, S, max_N, d, mode, mirror) || !q || !step) return hipErrorInvalidValue;
    const dim3 grid = guided_grid(max_N, d, B);
    if (mode == REUSE_STORE)
        hipLaunchKernelGGL((multistep_update_reuse_kernel<REUSE_STORE>), grid, dim3(256), 0, s, x2, eps, q, delta, *step, w, cu, prompt_len,
                           suffix_len, S, d, mirror);
    else
        hipLaunchKernelGGL((multistep_update_reuse_kernel<REUSE_LOAD>), grid, dim3(256), 0, s, x2, eps, q, delta, *step, w, cu, prompt_len,
                           suffix_len, S, d, mirror);
    return hipGetLastError();
}

}  // namespace ditto
