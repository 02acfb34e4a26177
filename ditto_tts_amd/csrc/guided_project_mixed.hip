// guided_project_mixed.hip — projected guidance (APG; include/ditto_project.h states the arithmetic) over a request stream's step
// (gfx950): guided_mixed.hip's layout and guided_project.hip's arithmetic.  The B utterances sit in rows [0, S) of x2 / eps2 and the G
// guided ones have their unconditional copies compacted behind them in rows [S, S + S_G); dir fp32 [S, d] is row-aligned with rows
// [0, S).  Every utterance stands at its own step of its own schedule, so a step holds three kinds side by side; kind[b] says which:
//   3 projected  launch 1: dd = ke (c - u), u read at the copy's rows, m' kept in dir, S_mm, S_mD, S_DD in fp64; the finish:
//                pcoef[b] = (fx, fc, fd, 0); launch 2: e = fmaf(fx, x, fmaf(fc, c, fd m')), x' to b's rows and the copy's
//   1 guided     launch 2 alone: e = fmaf(w, c - u, u), x' to both: guided_update_mixed_kernel's partner branch
//   0 plain      launch 2 alone: e = c, x' to b's rows                          (2 is never used here: hip.KIND_REUSE; others count as 0)
// A 1 or 3 without a usable partner (mixed_span's g < 0) counts as 0.  Three kernels over guided_update.h's mixed_span:
//   guidance_project_partial_mixed_kernel  guidance_project_partial_kernel's body with the window from mixed_span and u at sp.urow:
//       the chunk cut, the lane order and the butterfly are guided_project.h's, shared with the closed kernel; the four waves meet in
//       index order through LDS as there.  Workgroups of kinds 0 and 1 leave on the uniform branch: nothing of x2, eps2 or dir is read
//   guidance_project_finish_mixed_kernel   guidance_project_finish_kernel's statements for kind 3; pcoef[b] = (0, 1, 0, 0) otherwise
//   guided_update_project_mixed_kernel     project_rows (kind 3), update_rows<EPS_CFG> (kind 1), update_rows<EPS_COND> (kind 0) with the
//       DDIM line and per-utterance tags: no Philox draw where cz[b] == 0.  Kinds 0 and 1 neither read nor write dir
// The closed kernels are held to their machine code (tools/asm_identity.py), so the LDS meeting and the finish are restated here
// statement for statement instead of being moved out of them; tests/test_gpu_project_mixed_kernel.py holds the two to the same bits.
// b = blockIdx.y (blockIdx.x in the finish) is uniform: kind, partner, offsets and coefficients come in through scalar loads, the
// branches are scalar, every lane access is 16 bytes.  HBM traffic per generated element: projected 16 - 20 B in launch 1 (x, c, u and
// m with use_prev read; m' written) and 20 B in launch 2 (x, c, m' read; x' and the copy written); guided 20 B, plain 12 B, both in
// launch 2 alone; + 4 B each with a noise buffer; 0 B per prompt element.
#include "guided_project.h"

namespace ditto {

enum { KIND_PLAIN = 0, KIND_CFG = 1, KIND_PROJECT = 3 };

// kind[b] after its clamps: 0, 1 or 3; g = mixed_span's partner
__device__ __forceinline__ int project_kind(const int32_t* kind, int b, int g) {
    const int kd = kind[b];
    return g >= 0 && (kd == KIND_CFG || kd == KIND_PROJECT) ? kd : KIND_PLAIN;
}

// mixed_span's clamps: b's generated rows lie inside [0, S) — so do dir's, which share their offset — and the copy's inside
// [S, S + S_G).  A bad cu / partner / kind / prompt_len gives wrong rows, never an access outside x2, eps2 [S + S_G, d] or dir [S, d];
// the partials of utterance b stay inside its own `slots` of the scratch (project_chunks)
__global__ __launch_bounds__(256) void guidance_project_partial_mixed_kernel(ProjectMixedArgs a) {
    __shared__ double red[4][3];
    const int b = blockIdx.y;
    const MixedSpan sp = mixed_span(a.cu, a.partner, a.prompt_len, b, a.B, a.G, a.S, a.S_G, a.d);     // (guided_update.h)
    if (project_kind(a.kind, b, sp.g) != KIND_PROJECT) return;
    const size_t nchunk = project_chunks(sp.n4, a.slots);
    const ::ditto_project_coef k = a.proj[b];
    const f32x4* xc = reinterpret_cast<const f32x4*>(a.x2) + sp.base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(a.eps2) + sp.base4;
    const f32x4* eu = reinterpret_cast<const f32x4*>(a.eps2) + (size_t)sp.urow * (size_t)(a.d / 4);
    f32x4* mp = reinterpret_cast<f32x4*>(a.dir) + sp.base4;
    const int wave = threadIdx.x >> 6;
    for (size_t j = blockIdx.x; j < nchunk; j += gridDim.x) {
        double acc[3] = {0.0, 0.0, 0.0};
        if (k.use_prev) project_chunk<true>(xc, ec, eu, mp, j, sp.n4, k, acc);
        else project_chunk<false>(xc, ec, eu, mp, j, sp.n4, k, acc);
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

__global__ __launch_bounds__(64) void guidance_project_finish_mixed_kernel(ProjectMixedArgs a) {
#pragma clang fp contract(off)      // the finish as written: no product is fused into a neighbouring sum
    const int b = blockIdx.x, lane = threadIdx.x;
    const MixedSpan sp = mixed_span(a.cu, a.partner, a.prompt_len, b, a.B, a.G, a.S, a.S_G, a.d);
    float fx = 0.f, fc = 1.f, fd = 0.f;
    if (project_kind(a.kind, b, sp.g) == KIND_PROJECT) {
        const size_t nchunk = project_chunks(sp.n4, a.slots);
        const ::ditto_project_coef k = a.proj[b];
        const f64x2* part = reinterpret_cast<const f64x2*>(a.partial + (size_t)b * a.slots * 4);
        double acc[3] = {0.0, 0.0, 0.0};
        for (size_t j = lane; j < nchunk; j += 64) {            // an order that depends on the chunk count only
            const f64x2 p0 = part[2 * j], p1 = part[2 * j + 1];
            acc[0] += p0[0], acc[1] += p0[1], acc[2] += p1[0];
        }
        project_butterfly(acc);
        if (k.ke != 0.f) {
            const double n = 4.0 * (double)sp.n4;
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
    }
    if (lane == 0) reinterpret_cast<f32x4*>(a.pcoef)[b] = f32x4{fx, fc, fd, 0.f};
}

// NOISE and the Philox index: guided_update_mixed_kernel's (guided_mixed.hip): tags per utterance, no draw where cz[b] == 0
template <int NOISE>
__global__ __launch_bounds__(256) void guided_update_project_mixed_kernel(
    float* __restrict__ x2, const float* __restrict__ eps2, const float* __restrict__ dir, const float* __restrict__ pcoef,
    const float* __restrict__ noise, const int64_t* __restrict__ seeds, const unsigned* __restrict__ tags, const float* __restrict__ w,
    const float* __restrict__ a, const float* __restrict__ ce, const float* __restrict__ cz, const int32_t* __restrict__ cu,
    const int32_t* __restrict__ partner, const int32_t* __restrict__ kind, const int32_t* __restrict__ prompt_len, int B, int G, int S,
    int S_G, int d) {
    const int b = blockIdx.y;
    const MixedSpan sp = mixed_span(cu, partner, prompt_len, b, B, G, S, S_G, d);
    const int kd = project_kind(kind, b, sp.g);
    const GuidedCoef k = guided_coef<NOISE, true>(a, ce, cz, w, seeds, b);
    const unsigned tag = NOISE == 2 ? tags[b] : 0u;
    f32x4* xc = reinterpret_cast<f32x4*>(x2) + sp.base4;
    const f32x4* ec = reinterpret_cast<const f32x4*>(eps2) + sp.base4;
    const DdimLine<NOISE> ddim = {reinterpret_cast<const f32x4*>(noise) + sp.base4, k, tag, k.cz != 0.f};
    const size_t i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t ub4 = (size_t)sp.urow * (size_t)(d / 4);         // used with a partner only (kinds 1 and 3)
    if (kd == KIND_PROJECT) {
        const f32x4 f = reinterpret_cast<const f32x4*>(pcoef)[b];
        project_rows(xc, reinterpret_cast<f32x4*>(x2) + ub4, ec, reinterpret_cast<const f32x4*>(dir) + sp.base4, ddim, f, sp.n4, i0,
                     stride);
    } else if (kd == KIND_CFG) {
        update_rows<EPS_CFG, false>(xc, reinterpret_cast<f32x4*>(x2) + ub4, ec, reinterpret_cast<const f32x4*>(eps2) + ub4, ddim,
                                    nullptr, k.w, false, sp.n4, sp.n4, i0, stride);
    } else {
        update_rows<EPS_COND, false>(xc, xc, ec, ec, ddim, nullptr, k.w, false, sp.n4, sp.n4, i0, stride);
    }
}

static bool project_mixed_shape_ok(int B, int G, int S, int S_G, int max_N, int d) {
    return d > 0 && d % 64 == 0 && B > 0 && S > 0 && max_N > 0 && B <= 65535 && mixed_layout_ok(B, G, S, S_G);
}

hipError_t launch_guidance_project_mixed(const ProjectMixedArgs& a, int max_N, hipStream_t s) {
    // (the conditions of check_project_mixed, ditto_api.hip, which every public entry passes through first)
    if (!project_mixed_shape_ok(a.B, a.G, a.S, a.S_G, max_N, a.d) || !a.x2 || !a.eps2 || !a.dir || !a.proj || !a.pcoef || !a.partial ||
        !a.cu || !a.partner || !a.kind || a.slots < 1)
        return hipErrorInvalidValue;
    size_t gx = guidance_rescale_chunks(max_N, a.d);
    if (gx > (size_t)a.slots) gx = (size_t)a.slots;
    if (gx > 1024) gx = 1024;                                   // a longer utterance: its columns stride
    hipLaunchKernelGGL(guidance_project_partial_mixed_kernel, dim3((unsigned)gx, a.B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(guidance_project_finish_mixed_kernel, dim3(a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_guided_update_project_mixed(float* x2, const float* eps2, const float* dir, const float* pcoef, const float* noise,
                                              const int64_t* seeds, const unsigned* tags, const float* w, const float* a,
                                              const float* ce, const float* cz, const int32_t* cu, const int32_t* partner,
                                              const int32_t* kind, const int32_t* prompt_len, int B, int G, int S, int S_G, int max_N,
                                              int d, hipStream_t s) {
    if (!project_mixed_shape_ok(B, G, S, S_G, max_N, d) || !x2 || !eps2 || !dir || !pcoef || !w || !a || !ce ||
        ((noise || seeds) && !cz) || !cu || !partner || !kind || (noise && seeds) || (seeds && !tags))
        return hipErrorInvalidValue;
    const dim3 grid = guided_grid(max_N, d, B);
    noise_dispatch(noise, seeds, [&](auto nz) {
        hipLaunchKernelGGL((guided_update_project_mixed_kernel<decltype(nz)::value>), grid, dim3(256), 0, s, x2, eps2, dir, pcoef, noise,
                           seeds, tags, w, a, ce, cz, cu, partner, kind, prompt_len, B, G, S, S_G, d);
    });
    return hipGetLastError();
}

}  // namespace ditto
