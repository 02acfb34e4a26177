// guided_reuse.hip — the packed guided updates that keep and reuse the guidance direction (gfx950): the unconditional forward runs
// only at every k-th guided step (the "CFG cache" of FasterCache, Lv et al. 2024, without its frequency reweighting), and the steps in
// between add the last direction delta = c - u to the conditional prediction of the moment:
//   u + w (c - u) = c + (w - 1)(c - u)  ~  c_now + (w - 1) delta_last
// delta fp32 [S, d] is row-aligned with the conditional half.  Over guided_update.h's span and grid, like guided_packed.hip and
// guided_multistep.hip: grid (chunks, B), 256 threads, 16-byte lane accesses, b = blockIdx.y uniform over the workgroup, d % 64 == 0;
// the context rows of x2, eps, delta, q and a noise buffer are neither read nor written.
//   STORE (a refresh step; eps [2S, d]):   dl = c - u,  e = fmaf(w, dl, u),  delta = dl       guided_update.h's CFG expression: x' (and
//                                          q) get the bits of the CFG instantiations of the existing kernels, written to both halves
//   LOAD  (a reuse step;  eps [S, d]):     e = fmaf(w - 1, delta, c)                          delta is read and never written; x' goes
//                                          to the conditional half and, with the run-time `mirror`, to the row + S of the other
// then the DDIM line x' = fmaf(a, x, fmaf(ce, e, cz z)) with the scalar-tag noise (every utterance draws, window-local Philox index),
// or the multistep lines of guided_multistep.hip.  HBM-bound, per generated element: STORE the CFG update's bytes + 4 (20 + 4 DDIM
// without a noise buffer, 28 + 4 multistep with history); LOAD x, c and delta read (12 B) and x' written (4 B), 4 B more than the unguided
// update, + 4 B noise buffer, + 4 B mirror, + 8 B multistep history (q read and written).
#include "ditto_hip.h"
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

enum { REUSE_STORE = 1, REUSE_LOAD = 2 };

// the guided prediction of one element from the direction dv: c - u of this step at a refresh, the kept one at a reuse
template <int MODE> __device__ __forceinline__ float reuse_eps(float w, float wm1, float c, float u, float dv) {
    return MODE == REUSE_STORE ? fmaf(w, dv, u) : fmaf(wm1, dv, c);
}

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
            const float ev = reuse_eps<MODE>(k.w, wm1, c[e], u[e], dv);
            dl[e] = dv;
            o[e] = fmaf(k.a, xv[e], fmaf(k.ce, ev, k.cz * zv[e]));
        }
        xc[i] = o;
        if (both) xu[i] = o;
        if (MODE == REUSE_STORE) dp[i] = dl;
    }
}

// guided_multistep.hip's p, o, q lines behind the same two modes.  PREV false: q is written and never read
template <int MODE, bool PREV>
__device__ __forceinline__ void multistep_reuse_rows(f32x4* xc, f32x4* xu, const f32x4* ec, const f32x4* eu, f32x4* qp, f32x4* dp,
                                                     const ditto_multistep_coef& k, bool both, size_t n4, size_t i0, size_t stride) {
    const float wm1 = k.w - 1.0f;
    for (size_t i = i0; i < n4; i += stride) {
        const f32x4 xv = xc[i];
        const f32x4 c = ec[i];
        f32x4 u = c, dl;
        if (MODE == REUSE_STORE) u = eu[i];
        else dl = dp[i];
        f32x4 qv = {0.f, 0.f, 0.f, 0.f};
        if (PREV) qv = qp[i];
        f32x4 o, p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dv = MODE == REUSE_STORE ? c[e] - u[e] : dl[e];
            const float ev = reuse_eps<MODE>(k.w, wm1, c[e], u[e], dv);
            dl[e] = dv;
            p[e] = fmaf(k.kx, xv[e], k.ke * ev);
            o[e] = fmaf(k.a, xv[e], fmaf(k.b, p[e], PREV ? k.g * qv[e] : 0.f));
        }
        xc[i] = o;
        if (both) xu[i] = o;
        qp[i] = p;
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
    const bool both = MODE == REUSE_STORE || mirror != 0;
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (k.use_prev)
        multistep_reuse_rows<MODE, true>(xc, xc + half4, ec, ec + half4, qp, dp, k, both, ws.g4, i0, stride);
    else
        multistep_reuse_rows<MODE, false>(xc, xc + half4, ec, ec + half4, qp, dp, k, both, ws.g4, i0, stride);
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
    auto by_mode = [&](auto nz) {
        mode == REUSE_STORE ? go(nz, std::integral_constant<int, REUSE_STORE>{}) : go(nz, std::integral_constant<int, REUSE_LOAD>{});
    };
    seeds ? by_mode(std::integral_constant<int, 2>{}) : noise ? by_mode(std::integral_constant<int, 1>{})
                                                               : by_mode(std::integral_constant<int, 0>{});
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
