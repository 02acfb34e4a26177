// span_train.hip — span-masked training on a packed batch (gfx950): the forward diffusion that leaves each utterance's context rows
// clean, and the MSE over the generated rows with its gradient.  The span is window_span's window [cu[b] + P_b, cu[b+1] - Q_b)
// (guided_update.h; prompt_len, suffix_len: either may be NULL): a speech prompt in front, and for infilling objectives clean context
// behind as well.  Both kernels walk the WHOLE utterance, so the lane-to-quad assignment, the partial layout and the reduction tree,
// and with them the loss's bits, do not depend on where the window lies.  Elementwise, 16-byte lane accesses, grid (chunks, B) like
// the guided kernels; no atomics: the loss is reduced through per-workgroup partials summed in index order.
#include "common.h"
#include "guided_update.h"
#include "kernels.h"
#include "philox.h"

namespace ditto {

// x_in = x0 on the context rows (a bit copy), fmaf(ca[b], x0, cs[b] z) on the generated rows.  z: the packed buffer `noise` [S, d]
// (its context rows are never read), or SEEDED Philox of (seeds[b], tag) at the window-local quad index i - p4 — ditto_noise_normal's
// numbers for an utterance of G_b rows.  8 B per element seeded, 12 B with a buffer.
template <bool SEEDED>
__global__ __launch_bounds__(256) void span_noise_packed_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                                const int64_t* __restrict__ seeds, unsigned tag,
                                                                const float* __restrict__ ca, const float* __restrict__ cs,
                                                                const int32_t* __restrict__ cu, const int32_t* __restrict__ prompt_len,
                                                                const int32_t* __restrict__ suffix_len, float* __restrict__ x_in, int S,
                                                                int d) {
    const int b = blockIdx.y;
    const WindowSpan r = window_span(cu, prompt_len, suffix_len, b, S, d);
    const float a = ca[b], s = cs[b];
    const unsigned long long seed = SEEDED ? (unsigned long long)seeds[b] : 0ull;
    const f32x4* xp = reinterpret_cast<const f32x4*>(x0) + r.base4;
    const f32x4* zp = reinterpret_cast<const f32x4*>(noise) + r.base4;
    f32x4* op = reinterpret_cast<f32x4*>(x_in) + r.base4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < r.n4; i += stride) {
        f32x4 o = xp[i];
        if (i - r.p4 < r.g4) {                        // p4 <= i < p4 + g4, in one unsigned compare
            const f32x4 z = SEEDED ? normal4(seed, tag, i - r.p4) : zp[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaf(a, o[e], s * z[e]);
        }
        op[i] = o;
    }
}

// grad_eps = scale2 (eps - z) on the generated rows, exactly 0 on the context rows (eps is not read there); partial[b gridDim.x +
// blockIdx.x] = this workgroup's sum of (eps - z)^2, lanes in a fixed tree.  z as in span_noise_packed_kernel: SEEDED, the noise is
// regenerated and never exists in memory (eps read, grad written: 8 B per element).
template <bool SEEDED>
__global__ __launch_bounds__(256) void span_mse_packed_kernel(const float* __restrict__ eps, const float* __restrict__ noise,
                                                              const int64_t* __restrict__ seeds, unsigned tag,
                                                              const int32_t* __restrict__ cu, const int32_t* __restrict__ prompt_len,
                                                              const int32_t* __restrict__ suffix_len, float scale2,
                                                              float* __restrict__ grad, float* __restrict__ partial, int S, int d) {
    __shared__ float red[256];
    const int b = blockIdx.y;
    const WindowSpan r = window_span(cu, prompt_len, suffix_len, b, S, d);
    const unsigned long long seed = SEEDED ? (unsigned long long)seeds[b] : 0ull;
    const f32x4* ep = reinterpret_cast<const f32x4*>(eps) + r.base4;
    const f32x4* zp = reinterpret_cast<const f32x4*>(noise) + r.base4;
    f32x4* gp = reinterpret_cast<f32x4*>(grad) + r.base4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float acc = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < r.n4; i += stride) {
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (i - r.p4 < r.g4) {                        // p4 <= i < p4 + g4, in one unsigned compare
#pragma clang fp contract(off)      // eps - z must not fuse with the Box-Muller product r cos: the seeded mode gives the buffer mode's bits
            const f32x4 e = ep[i];
            const f32x4 z = SEEDED ? normal4(seed, tag, i - r.p4) : zp[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float df = e[k] - z[k];
                acc = fmaf(df, df, acc);
                g[k] = scale2 * df;
            }
        }
        gp[i] = g;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

// span_mse_packed_kernel for the v objective (Salimans & Ho 2022): target = fmaf(ca[b], z, -(cs[b] x0)), diff = pred - target,
// grad = (scale2 lw[b]) diff on the generated rows and exactly 0 on the context rows (pred, x0 and noise are not read there);
// partial[b gridDim.x + blockIdx.x] = lw[b] x this workgroup's sum of diff^2, the same lanes in the same tree — an utterance has one
// weight, so it multiplies the workgroup's sum once.  lw NULL: weight 1.  With ca = 1, cs = 0, weight 1 and a finite x0 the target
// is fmaf(1, z, -0) = z and every product by 1 is exact: grad and partials are span_mse_packed_kernel's bits.  One stream more than
// that kernel (x0): 12 B per element SEEDED, 16 B with a noise buffer.
template <bool SEEDED>
__global__ __launch_bounds__(256) void span_vloss_packed_kernel(const float* __restrict__ pred, const float* __restrict__ x0,
                                                                const float* __restrict__ noise, const int64_t* __restrict__ seeds,
                                                                unsigned tag, const float* __restrict__ ca, const float* __restrict__ cs,
                                                                const float* __restrict__ lw, const int32_t* __restrict__ cu,
                                                                const int32_t* __restrict__ prompt_len,
                                                                const int32_t* __restrict__ suffix_len, float scale2,
                                                                float* __restrict__ grad, float* __restrict__ partial, int S, int d) {
    __shared__ float red[256];
    const int b = blockIdx.y;
    const WindowSpan r = window_span(cu, prompt_len, suffix_len, b, S, d);
    const float a = ca[b], s = cs[b], wt = lw ? lw[b] : 1.f;
    const float gscale = scale2 * wt;
    const unsigned long long seed = SEEDED ? (unsigned long long)seeds[b] : 0ull;
    const f32x4* pp = reinterpret_cast<const f32x4*>(pred) + r.base4;
    const f32x4* xp = reinterpret_cast<const f32x4*>(x0) + r.base4;
    const f32x4* zp = reinterpret_cast<const f32x4*>(noise) + r.base4;
    f32x4* gp = reinterpret_cast<f32x4*>(grad) + r.base4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float acc = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < r.n4; i += stride) {
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (i - r.p4 < r.g4) {                        // p4 <= i < p4 + g4, in one unsigned compare
#pragma clang fp contract(off)      // only the written fmafs fuse: the Box-Muller product r cos and cs x0 round on their own
            const f32x4 p = pp[i];
            const f32x4 x = xp[i];
            const f32x4 z = SEEDED ? normal4(seed, tag, i - r.p4) : zp[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float sx = s * x[k];
                const float df = p[k] - fmaf(a, z[k], -sx);
                acc = fmaf(df, df, acc);
                g[k] = gscale * df;
            }
        }
        gp[i] = g;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = red[0] * wt;
}

// loss = inv_n * (the partials summed in index order): lane l sums its contiguous share in order, lane 0 the 256 shares in order
__global__ __launch_bounds__(256) void span_mse_finish_kernel(const float* __restrict__ partial, size_t n_partial, float inv_n,
                                                              float* __restrict__ loss) {
    __shared__ float red[256];
    const size_t per = (n_partial + 255) / 256, lo = threadIdx.x * per, hi = lo + per < n_partial ? lo + per : n_partial;
    float acc = 0.f;
    for (size_t i = lo; i < hi; ++i) acc += partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int l = 0; l < 256; ++l) t += red[l];
        loss[0] = t * inv_n;
    }
}

size_t span_mse_partials(int B, int max_N, int d) { return (size_t)B * guided_grid(max_N, d, B).x; }

hipError_t launch_span_noise_packed(const float* x0, const float* noise, const int64_t* seeds, unsigned tag, const float* ca,
                                    const float* cs, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len,
                                    float* x_in, int B, int S, int max_N, int d, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || (!noise == !seeds)) return hipErrorInvalidValue;
    if (seeds)
        hipLaunchKernelGGL(span_noise_packed_kernel<true>, guided_grid(max_N, d, B), dim3(256), 0, s, x0, noise, seeds, tag, ca, cs, cu,
                           prompt_len, suffix_len, x_in, S, d);
    else
        hipLaunchKernelGGL(span_noise_packed_kernel<false>, guided_grid(max_N, d, B), dim3(256), 0, s, x0, noise, seeds, tag, ca, cs, cu,
                           prompt_len, suffix_len, x_in, S, d);
    return hipGetLastError();
}

hipError_t launch_span_mse_packed(const float* eps, const float* noise, const int64_t* seeds, unsigned tag, const int32_t* cu,
                                  const int32_t* prompt_len, const int32_t* suffix_len, double n_elems, float* grad, float* loss,
                                  float* partial, int B, int S, int max_N, int d, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || (!noise == !seeds) || !(n_elems >= 1.0))
        return hipErrorInvalidValue;
    const float scale2 = (float)(2.0 / n_elems), inv_n = (float)(1.0 / n_elems);
    const dim3 grid = guided_grid(max_N, d, B);
    if (seeds)
        hipLaunchKernelGGL(span_mse_packed_kernel<true>, grid, dim3(256), 0, s, eps, noise, seeds, tag, cu, prompt_len, suffix_len,
                           scale2, grad, partial, S, d);
    else
        hipLaunchKernelGGL(span_mse_packed_kernel<false>, grid, dim3(256), 0, s, eps, noise, seeds, tag, cu, prompt_len, suffix_len,
                           scale2, grad, partial, S, d);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(span_mse_finish_kernel, dim3(1), dim3(256), 0, s, partial, (size_t)B * grid.x, inv_n, loss);
    return hipGetLastError();
}

hipError_t launch_span_vloss_packed(const float* pred, const float* x0, const float* noise, const int64_t* seeds, unsigned tag,
                                    const float* ca, const float* cs, const float* lw, const int32_t* cu, const int32_t* prompt_len,
                                    const int32_t* suffix_len, double n_elems, float* grad, float* loss, float* partial, int B, int S,
                                    int max_N, int d, hipStream_t s) {
    if (d % 64 || B <= 0 || S <= 0 || max_N <= 0 || B > 65535 || !cu || !x0 || !ca || !cs || (!noise == !seeds) || !(n_elems >= 1.0))
        return hipErrorInvalidValue;
    const float scale2 = (float)(2.0 / n_elems), inv_n = (float)(1.0 / n_elems);
    const dim3 grid = guided_grid(max_N, d, B);       // span_mse_packed's grid: the same partial layout and workspace
    if (seeds)
        hipLaunchKernelGGL(span_vloss_packed_kernel<true>, grid, dim3(256), 0, s, pred, x0, noise, seeds, tag, ca, cs, lw, cu, prompt_len,
                           suffix_len, scale2, grad, partial, S, d);
    else
        hipLaunchKernelGGL(span_vloss_packed_kernel<false>, grid, dim3(256), 0, s, pred, x0, noise, seeds, tag, ca, cs, lw, cu, prompt_len,
                           suffix_len, scale2, grad, partial, S, d);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(span_mse_finish_kernel, dim3(1), dim3(256), 0, s, partial, (size_t)B * grid.x, inv_n, loss);
    return hipGetLastError();
}

}  // namespace ditto
