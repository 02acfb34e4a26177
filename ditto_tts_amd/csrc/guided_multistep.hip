// guided_multistep.hip — the packed guided update of the second-order multistep data-prediction solver, DPM-Solver++(2M) (Lu et al.
// 2022), for gfx950.  One forward per step like the strided (DDIM) update; the extra state is the previous step's x0 prediction per
// generated row, kept in a second fp32 buffer q [S, d].  Over guided_update.h's span and grid, like guided_packed.hip.
// The row loop is guided_update.h's update_rows with its MultistepLine:
//   e  = CFG ? fmaf(w, c - u, u) : c                       (EPS_CFG / EPS_COND)
//   x0 = fmaf(kx, x, ke * e)                               the data prediction: kx = 1 / alpha, ke = -sigma / alpha
//   x' = fmaf(a, x, fmaf(b, x0, use_prev ? g * q : 0))     written to the conditional and, under CFG, the unconditional half of x2
//   q  = x0
// Deterministic: no noise term.  HBM-bound: per generated element under CFG x, c, u, q read and both halves and q written, 28 B (24 B
// at a step without history; without CFG 16 + 4 B); 16-byte lane accesses, grid (chunks, B); d % 64 == 0: no quad straddles a row.
#include "ditto_hip.h"
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

// PER_UTT false: every utterance stands at the step `step` (a kernel argument; its w is not used: w[b] is the guidance scale).
// PER_UTT true: utterance b at coefs[b], guidance scale included (a request stream: each utterance at its own index of its own
// schedule).  b = blockIdx.y is uniform over the workgroup: the block comes in through scalar loads and the use_prev branch is
// uniform.  The update runs over window_span's window [cu[b] + P_b, cu[b+1] - Q_b) (prompt_len, suffix_len: either may be NULL): the
// clean context rows of x2, eps2 and q are neither read nor written, on either side.
template <bool CFG, bool PER_UTT>
__global__ __launch_bounds__(256) void multistep_update_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                               float* __restrict__ q, ditto_multistep_coef step,
                                                               const ditto_multistep_coef* __restrict__ coefs,
                                                               const float* __restrict__ w, const int32_t* __restrict__ cu,
                                                               const int32_t* __restrict__ prompt_len,
                                                               const int32_t* __restrict__ suffix_len, int S, int d) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);     // (guided_update.h)
    const size_t base4 = ws.base4 + ws.p4;
    ditto_multistep_coef k = step;
    if (PER_UTT) k = coefs[b];
    else k.w = CFG ? w[b] : 0.f;
    const size_t half4 = (size_t)S * d / 4;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + base4;
    f32x4* qp = reinterpret_cast<f32x4*>(q) + base4;
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    constexpr int MODE = CFG ? EPS_CFG : EPS_COND;
    if (k.use_prev)
        update_rows<MODE, false>(xc, xc + half4, ec, ec + half4, MultistepLine<true>{qp, k}, nullptr, k.w, false, ws.g4, ws.g4, i0, stride);
    else
        update_rows<MODE, false>(xc, xc + half4, ec, ec + half4, MultistepLine<false>{qp, k}, nullptr, k.w, false, ws.g4, ws.g4, i0, stride);
}

hipError_t launch_multistep_update_packed(float* x2, const float* eps2, float* q, const ditto_multistep_coef* step,
                                          const ditto_multistep_coef* coefs, const float* w, const int32_t* cu,
                                          const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, bool cfg,
                                          hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || !q || !step == !coefs || (step && cfg && !w))
        return hipErrorInvalidValue;
    const dim3 grid = guided_grid(max_N, d, B);
    const ditto_multistep_coef none = {};
    auto go = [&](auto cf, auto pu) {
        hipLaunchKernelGGL((multistep_update_kernel<decltype(cf)::value, decltype(pu)::value>), grid, dim3(256), 0, s, x2, eps2, q,
                           step ? *step : none, coefs, w, cu, prompt_len, suffix_len, S, d);
    };
    if (cfg) coefs ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
    else coefs ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
    return hipGetLastError();
}

}  // namespace ditto
