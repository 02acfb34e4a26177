// guided_rescale.hip — guidance rescale for packed guided sampling (gfx950): Lin et al. 2024, "Common Diffusion Noise Schedules and
// Sample Steps are Flawed", section 3.4.  At a strong guidance scale w the guided prediction e = u + w (c - u) has a much larger
// standard deviation than the conditional prediction c; the rescale multiplies e by
//   s_b = 1 + phi_b (sigma_c / sigma_e - 1)          sigma over the generated rows of utterance b, all d columns, population form
// Every update kernel reads its coefficients per utterance from device memory and x' is linear in e, so s_b e is the EXISTING update
// run with ce[b] s_b (2M solver: ke s_b).  The work here is the one thing that is not elementwise: a per-utterance reduction that
// patches a coefficient array.  Two launches, no atomics:
//   guidance_rescale_partial_kernel  grid (chunk columns, B): chunk j of utterance b = quads [j CHUNK, (j + 1) CHUNK) of its OWN
//       generated region (CHUNK = DITTO_RESCALE_CHUNK_QUADS, kernels.h).  Lane l reads quads j CHUNK + l, + 256, ... (16-byte loads of c
//       and u, coalesced), e_i = fmaf(w, c_i - u_i, u_i) in fp32 — guided_rows' expression —, and adds c, c^2, e, e^2 into four fp64
//       accumulators serially; the 64 lanes of a wave meet in a fixed xor butterfly, the 4 waves in index order through LDS; 4 doubles
//       per chunk go to the scratch.  A column strides over chunk indices when the grid has fewer columns than the utterance has
//       chunks: the partials are the same.
//   guidance_rescale_finish_kernel   one wave per utterance: lane l adds partials l, l + 64, ... in order, the same butterfly, then
//       mean and variance, r = sqrt(var_c / var_e), s = 1 + phi (r - 1) in fp64, s32 = (float)s; scale[b] = s32 and coef_out[b] =
//       coef_in[b] * s32 (one fp32 multiply).  s32 = 1 and coef_out a bit copy where the utterance is unguided (partner < 0), phi_b ==
//       0, var_e <= 0 or r is not finite; an unguided or phi == 0 utterance reads none of its eps.
// So s32 of an utterance is a function of its own generated rows, w_b and phi_b: not of its position, its neighbours, B, S, max_N or
// the grid.  HBM-bound: 8 B read per generated element of a rescaled utterance; the fp64 work is 6 instructions per element.
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

typedef __attribute__((ext_vector_type(2))) double f64x2;
constexpr int kChunk = DITTO_RESCALE_CHUNK_QUADS;
static_assert(kChunk % 1024 == 0, "a chunk is whole rounds of 4 quads per lane of 256 lanes");

// utterance b: its generated quads, where u sits, and whether anything is rescaled at all.  The spans are guided_update.h's — the
// rows the update that follows will read — in both layouts; phi is clamped into [0, 1] (NaN: 0)
struct RescaleSpan { size_t base4, n4, ub4; float phi; bool active; };
__device__ __forceinline__ RescaleSpan rescale_span(const RescaleArgs& a, int b) {
    RescaleSpan r;
    bool guided = true;
    if (a.partner) {
        const MixedSpan m = mixed_span(a.cu, a.partner, a.prompt_len, b, a.B, a.G, a.S, a.S_G, a.d);
        r.base4 = m.base4, r.n4 = m.n4, r.ub4 = (size_t)m.urow * ((size_t)a.d / 4);
        guided = m.g >= 0;
    } else {
        const GuidedSpan g = generated_span(a.cu, a.prompt_len, b, a.S, a.d);
        r.base4 = g.base4, r.n4 = g.n4, r.ub4 = g.base4 + (size_t)a.S * a.d / 4;
    }
    const float p = a.phi[b];
    r.phi = p > 0.f ? (p < 1.f ? p : 1.f) : 0.f;
    r.active = guided && r.phi > 0.f;
    return r;
}

__device__ __forceinline__ size_t rescale_chunks(const RescaleSpan& r, int slots) {
    const size_t n = (r.n4 + kChunk - 1) / kChunk;
    return n < (size_t)slots ? n : (size_t)slots;
}

// one quad of c and u into the four sums, element 0 .. 3 in order
__device__ __forceinline__ void rescale_add(const f32x4& c, const f32x4& u, float w, double (&acc)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ev = fmaf(w, c[e] - u[e], u[e]);
        const double cd = (double)c[e], ed = (double)ev;
        acc[0] += cd;
        acc[1] = fma(cd, cd, acc[1]);
        acc[2] += ed;
        acc[3] = fma(ed, ed, acc[3]);
    }
}

// the fixed cross-lane order: after it every lane of the wave holds the same four sums
__device__ __forceinline__ void rescale_butterfly(double (&acc)[4]) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], m, 64);
    }
}

__global__ __launch_bounds__(256) void guidance_rescale_partial_kernel(RescaleArgs a) {
    __shared__ double red[4][4];
    const int b = blockIdx.y;
    const RescaleSpan sp = rescale_span(a, b);
    if (!sp.active) return;                                     // (uniform) nothing of this utterance's eps is read
    const size_t nchunk = rescale_chunks(sp, a.slots);
    const float w = a.w[(size_t)b * a.cstride];
    const f32x4* ec = reinterpret_cast<const f32x4*>(a.eps2) + sp.base4;
    const f32x4* eu = reinterpret_cast<const f32x4*>(a.eps2) + sp.ub4;
    const int wave = threadIdx.x >> 6;
    for (size_t j = blockIdx.x; j < nchunk; j += gridDim.x) {
        const size_t q0 = j * kChunk + threadIdx.x;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if ((j + 1) * kChunk <= sp.n4) {                       // a whole chunk: 4 rounds of 4 + 4 loads in flight per lane
#pragma unroll 1
            for (int k0 = 0; k0 < kChunk / 256; k0 += 4) {
                f32x4 c[4], u[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    c[k] = ec[q0 + (size_t)(k0 + k) * 256];
                    u[k] = eu[q0 + (size_t)(k0 + k) * 256];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) rescale_add(c[k], u[k], w, acc);
            }
        } else {                                                // the utterance's last chunk: the same order, as far as it goes
            for (size_t q = q0; q < sp.n4; q += 256) rescale_add(ec[q], eu[q], w, acc);
        }
        rescale_butterfly(acc);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[wave][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
            f64x2* out = reinterpret_cast<f64x2*>(a.partial + ((size_t)b * a.slots + j) * 4);
            out[0] = f64x2{t[0], t[1]};
            out[1] = f64x2{t[2], t[3]};
        }
        __syncthreads();                                        // red is written again by the next chunk of this column
    }
}

__global__ __launch_bounds__(64) void guidance_rescale_finish_kernel(RescaleArgs a) {
#pragma clang fp contract(off)      // mean and variance as written: no product is fused into a neighbouring sum
    const int b = blockIdx.x, lane = threadIdx.x;
    const RescaleSpan sp = rescale_span(a, b);
    float s32 = 1.f;
    bool scaled = false;
    if (sp.active) {
        const size_t nchunk = rescale_chunks(sp, a.slots);
        const f64x2* part = reinterpret_cast<const f64x2*>(a.partial + (size_t)b * a.slots * 4);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (size_t j = lane; j < nchunk; j += 64) {            // an order that depends on the chunk count only
            const f64x2 p0 = part[2 * j], p1 = part[2 * j + 1];
            acc[0] += p0[0], acc[1] += p0[1], acc[2] += p1[0], acc[3] += p1[1];
        }
        rescale_butterfly(acc);
        const double n = 4.0 * (double)sp.n4;
        const double mc = acc[0] / n, me = acc[2] / n;
        double vc = acc[1] / n - mc * mc;
        const double ve = acc[3] / n - me * me;
        vc = vc > 0.0 ? vc : 0.0;
        if (ve > 0.0) {
            const double r = sqrt(vc / ve);
            if (r - r == 0.0) {                                 // finite
                s32 = (float)(1.0 + (double)sp.phi * (r - 1.0));
                scaled = true;
            }
        }
    }
    // the block of utterance b: `copy` words from koff words in front of its coefficient (a whole ditto_multistep_coef, or the one word)
    const unsigned* in = reinterpret_cast<const unsigned*>(a.coef_in + (size_t)b * a.cstride - a.koff);
    unsigned* out = reinterpret_cast<unsigned*>(a.coef_out + (size_t)b * a.cstride - a.koff);
    if (lane < a.copy) {
        unsigned v = in[lane];
        if (scaled && lane == a.koff) v = __float_as_uint(__uint_as_float(v) * s32);
        out[lane] = v;
    }
    if (lane == 0) a.scale[b] = s32;
}

size_t guidance_rescale_chunks(int max_N, int d) {
    const size_t n4 = (size_t)max_N * d / 4;
    return (n4 + kChunk - 1) / kChunk;
}

hipError_t launch_guidance_rescale(const RescaleArgs& a, int max_N, hipStream_t s) {
    // (the conditions of check_rescale, ditto_api.hip, which every public entry passes through first)
    if (a.d % 64 || a.B <= 0 || a.B > 65535 || a.S <= 0 || max_N <= 0 || !a.eps2 || !a.w || !a.phi || !a.coef_in || !a.coef_out ||
        !a.scale || !a.partial || !a.cu || a.slots < 1 || a.cstride < 1 || a.koff < 0 || a.copy < 1 || a.koff >= a.copy ||
        a.copy > 64 || (a.partner && !mixed_layout_ok(a.B, a.G, a.S, a.S_G)))
        return hipErrorInvalidValue;
    size_t gx = guidance_rescale_chunks(max_N, a.d);
    if (gx > (size_t)a.slots) gx = (size_t)a.slots;
    if (gx > 1024) gx = 1024;                                   // a longer utterance: its columns stride
    hipLaunchKernelGGL(guidance_rescale_partial_kernel, dim3((unsigned)gx, a.B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(guidance_rescale_finish_kernel, dim3(a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ditto
