// guided_project.hip — projected guidance for packed guided sampling (gfx950): Adaptive Projected Guidance, Sadat, Hilliges & Weber
// 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models", Algorithm 1.  The guidance direction is
// taken in x0 space (D = kx x + ke out), split into the part parallel to the conditional prediction D_c and the part orthogonal to it,
// and the parallel part is down-weighted by eta; the direction may be capped in size (r) and carry a momentum (beta) across steps.
// include/ditto_project.h states the arithmetic; this file is three kernels over guided_update.h's window span (their device functions
// — the chunk cut, one quad's arithmetic, a chunk's lane order, the butterfly, project_rows — live in guided_project.h, which
// guided_project_mixed.hip, the same over a request stream's layout, includes too):
//   guidance_project_partial_kernel  grid (chunk columns, B), guided_rescale.hip's cut: chunk j of utterance b = quads [j CHUNK, (j + 1)
//       CHUNK) of its OWN window.  Lane l reads quads j CHUNK + l, + 256, ... of x, c, u (and m with use_prev), 16 bytes each, forms
//       dd = ke (c - u), m' = use_prev ? fmaf(beta, m, dd) : dd, D = fmaf(kx, x, ke c) in fp32, stores m' and adds m'^2, m' D, D^2 into
//       three fp64 accumulators serially; a wave's 64 lanes meet in a fixed xor butterfly, the 4 waves in index order through LDS; 4
//       doubles per chunk (the last 0) go to the scratch.  A column strides over chunk indices when the grid has fewer columns than
//       the utterance has chunks: the partials are the same.
//   guidance_project_finish_kernel   one wave per utterance: lane l adds partials l, l + 64, ... in order, the same butterfly, then
//       rms, rho, p, kappa in fp64 and pcoef[b] = (fx, fc, fd, 0).
//   guided_update_project_kernel / multistep_update_project_kernel   e = fmaf(fx, x, fmaf(fc, c, fd m')), then guided_update.h's
//       DdimLine or MultistepLine, x' to both halves.  u is not read.
// The updates keep a row loop of their own (project_rows) instead of a fifth mode of update_rows: the guided prediction here takes
// three per-utterance factors where update_rows carries one (w), so a mode would change that function's signature and the text every
// other update kernel is compiled from — and those kernels are held to their machine code (tools/asm_identity.py).  The solver lines
// are guided_update.h's own, so x' given e has the plain entries' bits by construction.
// So an utterance's pcoef, m' and x' are functions of its own window and parameters: not of its position, its neighbours, B, S, max_N
// or the grid.  HBM-bound: launch 1 reads 12 - 16 B and writes 4 B per generated element (9 fp64 instructions per element); launch 2
// reads 12 B and writes 8 B (+ 4 B noise buffer, + 8 B multistep history).
#include "guided_project.h"

namespace ditto {

__global__ __launch_bounds__(256) void guidance_project_partial_kernel(ProjectArgs a) {
    __shared__ double red[4][3];
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(a.cu, a.prompt_len, a.suffix_len, b, a.S, a.d);     // (guided_update.h)
    const size_t base4 = ws.base4 + ws.p4, half4 = (size_t)a.S * a.d / 4;
    const size_t nchunk = project_chunks(ws.g4, a.slots);
    const ::ditto_project_coef k = a.proj[b];                  // b = blockIdx.y is uniform: scalar loads, a uniform use_prev branch
    const f32x4* xc = reinterpret_cast<const f32x4*>(a.x2) + base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(a.eps2) + base4;
    const f32x4* eu = ec + half4;
    f32x4* mp = reinterpret_cast<f32x4*>(a.dir) + base4;
    const int wave = threadIdx.x >> 6;
    for (size_t j = blockIdx.x; j < nchunk; j += gridDim.x) {
        double acc[3] = {0.0, 0.0, 0.0};
        if (k.use_prev) project_chunk<true>(xc, ec, eu, mp, j, ws.g4, k, acc);
        else project_chunk<false>(xc, ec, eu, mp, j, ws.g4, k, acc);
        project_butterfly(acc);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) red[wave][i] = acc[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double t[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
            f64x2* out = reinterpret_cast<f64x2*>(a.partial + ((size_t)b * a.slots + j) * 4);
            out[0] = f64x2{t[0], t[1]};
            out[1] = f64x2{t[2], 0.0};
        }
        __syncthreads();                                        // red is written again by the next chunk of this column
    }
}

__global__ __launch_bounds__(64) void guidance_project_finish_kernel(ProjectArgs a) {
#pragma clang fp contract(off)      // the finish as written: no product is fused into a neighbouring sum
    const int b = blockIdx.x, lane = threadIdx.x;
    const WindowSpan ws = window_span(a.cu, a.prompt_len, a.suffix_len, b, a.S, a.d);
    const size_t nchunk = project_chunks(ws.g4, a.slots);
    const ::ditto_project_coef k = a.proj[b];
    const f64x2* part = reinterpret_cast<const f64x2*>(a.partial + (size_t)b * a.slots * 4);
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t j = lane; j < nchunk; j += 64) {                // an order that depends on the chunk count only
        const f64x2 p0 = part[2 * j], p1 = part[2 * j + 1];
        acc[0] += p0[0], acc[1] += p0[1], acc[2] += p1[0];
    }
    project_butterfly(acc);
    float fx = 0.f, fc = 1.f, fd = 0.f;
    if (k.ke != 0.f) {
        const double n = 4.0 * (double)ws.g4;
        const double rms = sqrt(acc[0] / n), r = (double)k.r;
        double rho = 1.0;
        if (r > 0.0 && rms - rms == 0.0 && rms > r) rho = r / rms;
        double p = 0.0;
        if (acc[2] - acc[2] == 0.0 && acc[2] > 0.0) p = acc[1] / acc[2];
        const double eta = k.eta > 0.f ? (k.eta < 1.f ? (double)k.eta : 1.0) : 0.0;
        const double wr = ((double)k.w - 1.0) * rho;
        const double kappa = (wr * (1.0 - eta)) * p;
        fx = (float)((-kappa * (double)k.kx) / (double)k.ke);
        fc = (float)(1.0 - kappa);
        fd = (float)(wr / (double)k.ke);
    }
    if (lane == 0) reinterpret_cast<f32x4*>(a.pcoef)[b] = f32x4{fx, fc, fd, 0.f};
}

// NOISE, TAGS and the Philox index: guided_update_packed_kernel's (guided_packed.hip), to the letter
template <int NOISE, bool TAGS>
__global__ __launch_bounds__(256) void guided_update_project_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                    const float* __restrict__ dir, const float* __restrict__ pcoef,
                                                                    const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                                    unsigned step, const unsigned* __restrict__ tags,
                                                                    const float* __restrict__ a, const float* __restrict__ ce,
                                                                    const float* __restrict__ cz, const int32_t* __restrict__ cu,
                                                                    const int32_t* __restrict__ prompt_len,
                                                                    const int32_t* __restrict__ suffix_len, int S, int d) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);     // (guided_update.h)
    const size_t base4 = ws.base4 + ws.p4, half4 = (size_t)S * d / 4;
    const GuidedCoef k = guided_coef<NOISE, false>(a, ce, cz, nullptr, seeds, b);
    const f32x4 f = reinterpret_cast<const f32x4*>(pcoef)[b];
    const unsigned tag = TAGS ? (NOISE == 2 ? tags[b] : 0u) : step;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + base4;
    const DdimLine<NOISE> ddim = {reinterpret_cast<const f32x4*>(noise) + base4, k, tag, TAGS ? k.cz != 0.f : true};
    project_rows(xc, xc + half4, reinterpret_cast<const f32x4*>(eps2) + base4, reinterpret_cast<const f32x4*>(dir) + base4, ddim, f,
                 ws.g4, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// PER_UTT: multistep_update_kernel's (guided_multistep.hip); the step's w is not used
template <bool PER_UTT>
__global__ __launch_bounds__(256) void multistep_update_project_kernel(float* __restrict__ x2, const float* __restrict__ eps2,
                                                                       float* __restrict__ q, const float* __restrict__ dir,
                                                                       const float* __restrict__ pcoef, ditto_multistep_coef step,
                                                                       const ditto_multistep_coef* __restrict__ coefs,
                                                                       const int32_t* __restrict__ cu,
                                                                       const int32_t* __restrict__ prompt_len,
                                                                       const int32_t* __restrict__ suffix_len, int S, int d) {
    const int b = blockIdx.y;
    const WindowSpan ws = window_span(cu, prompt_len, suffix_len, b, S, d);     // (guided_update.h)
    const size_t base4 = ws.base4 + ws.p4, half4 = (size_t)S * d / 4;
    ditto_multistep_coef k = step;
    if (PER_UTT) k = coefs[b];
    const f32x4 f = reinterpret_cast<const f32x4*>(pcoef)[b];
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + base4;
    const f32x4* mp = reinterpret_cast<const f32x4*>(dir) + base4;
    f32x4* qp = reinterpret_cast<f32x4*>(q) + base4;
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (k.use_prev) project_rows(xc, xc + half4, ec, mp, MultistepLine<true>{qp, k}, f, ws.g4, i0, stride);
    else project_rows(xc, xc + half4, ec, mp, MultistepLine<false>{qp, k}, f, ws.g4, i0, stride);
}

static bool project_shape_ok(int B, int S, int max_N, int d) {
    return d > 0 && d % 64 == 0 && B > 0 && S > 0 && max_N > 0 && B <= 65535;
}

hipError_t launch_guidance_project(const ProjectArgs& a, int max_N, hipStream_t s) {
    // (the conditions of check_project, ditto_api.hip, which every public entry passes through first)
    if (!project_shape_ok(a.B, a.S, max_N, a.d) || !a.x2 || !a.eps2 || !a.dir || !a.proj || !a.pcoef || !a.partial || !a.cu ||
        a.slots < 1)
        return hipErrorInvalidValue;
    size_t gx = guidance_rescale_chunks(max_N, a.d);
    if (gx > (size_t)a.slots) gx = (size_t)a.slots;
    if (gx > 1024) gx = 1024;                                   // a longer utterance: its columns stride
    hipLaunchKernelGGL(guidance_project_partial_kernel, dim3((unsigned)gx, a.B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(guidance_project_finish_kernel, dim3(a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_guided_update_project(float* x2, const float* eps2, const float* dir, const float* pcoef, const float* noise,
                                        const int64_t* seeds, unsigned step, const unsigned* tags, const float* a, const float* ce,
                                        const float* cz, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                        int S, int max_N, int d, hipStream_t s) {
    if (!project_shape_ok(B, S, max_N, d) || !x2 || !eps2 || !dir || !pcoef || !a || !ce || ((noise || seeds) && !cz) || !cu ||
        (noise && seeds))
        return hipErrorInvalidValue;
    return noise_dispatch(noise, seeds, [&](auto nz) {
        auto go = [&](auto tg) {
            hipLaunchKernelGGL((guided_update_project_kernel<decltype(nz)::value, decltype(tg)::value>), guided_grid(max_N, d, B),
                               dim3(256), 0, s, x2, eps2, dir, pcoef, noise, seeds, tags ? 0u : step, tags, a, ce, cz, cu, prompt_len,
                               suffix_len, S, d);
        };
        tags ? go(std::true_type{}) : go(std::false_type{});
        return hipGetLastError();
    });
}

hipError_t launch_multistep_update_project(float* x2, const float* eps2, float* q, const float* dir, const float* pcoef,
                                           const ditto_multistep_coef* step, const ditto_multistep_coef* coefs, const int32_t* cu,
                                           const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d,
                                           hipStream_t s) {
    if (!project_shape_ok(B, S, max_N, d) || !x2 || !eps2 || !q || !dir || !pcoef || !cu || !step == !coefs) return hipErrorInvalidValue;
    const dim3 grid = guided_grid(max_N, d, B);
    const ditto_multistep_coef none = {};
    if (coefs)
        hipLaunchKernelGGL((multistep_update_project_kernel<true>), grid, dim3(256), 0, s, x2, eps2, q, dir, pcoef, none, coefs, cu,
                           prompt_len, suffix_len, S, d);
    else
        hipLaunchKernelGGL((multistep_update_project_kernel<false>), grid, dim3(256), 0, s, x2, eps2, q, dir, pcoef, *step, coefs, cu,
                           prompt_len, suffix_len, S, d);
    return hipGetLastError();
}

}  // namespace ditto
