// guided_project.h — the device functions the projected-guidance kernels of the closed layout (guided_project.hip) and of a request
// stream's mixed layout (guided_project_mixed.hip) are both compiled from: the chunk cut, one quad's arithmetic, the lane order of a
// chunk, the cross-lane butterfly and the row loop of the update.  One text, so an utterance's partial sums, its m' and its x' have
// the same bits in either layout by construction.  include/ditto_project.h states the arithmetic.
#pragma once
#include "ditto_project.h"
#include "guided_update.h"
#include "kernels.h"

namespace ditto {

typedef __attribute__((ext_vector_type(2))) double f64x2;
constexpr int kChunk = DITTO_RESCALE_CHUNK_QUADS;
static_assert(kChunk % 1024 == 0, "a chunk is whole rounds of 4 quads per lane of 256 lanes");
static_assert(sizeof(::ditto_project_coef) == 32, "ditto_project_coef is 32 bytes");

__device__ __forceinline__ size_t project_chunks(size_t n4, int slots) {
    const size_t n = (n4 + kChunk - 1) / kChunk;
    return n < (size_t)slots ? n : (size_t)slots;
}

// one quad into the direction and the three sums, element 0 .. 3 in order; returns m'
template <bool PREV>
__device__ __forceinline__ f32x4 project_add(const f32x4& x, const f32x4& c, const f32x4& u, const f32x4& m,
                                             const ::ditto_project_coef& k, double (&acc)[3]) {
    f32x4 mo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float dd = k.ke * (c[e] - u[e]);
        const float mv = PREV ? fmaf(k.beta, m[e], dd) : dd;
        const float dv = fmaf(k.kx, x[e], k.ke * c[e]);
        const double md = (double)mv, Dd = (double)dv;
        acc[0] = fma(md, md, acc[0]);
        acc[1] = fma(md, Dd, acc[1]);
        acc[2] = fma(Dd, Dd, acc[2]);
        mo[e] = mv;
    }
    return mo;
}

// the fixed cross-lane order: after it every lane of the wave holds the same three sums
__device__ __forceinline__ void project_butterfly(double (&acc)[3]) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += __shfl_xor(acc[k], m, 64);
    }
}

// one chunk's quads of one lane: a whole chunk keeps 4 rounds of loads in flight, the last chunk runs the same order as far as it goes
template <bool PREV>
__device__ __forceinline__ void project_chunk(const f32x4* xc, const f32x4* ec, const f32x4* eu, f32x4* mp, size_t j, size_t n4,
                                              const ::ditto_project_coef& k, double (&acc)[3]) {
    const size_t q0 = j * kChunk + threadIdx.x;
    if ((j + 1) * kChunk <= n4) {
#pragma unroll 1
        for (int k0 = 0; k0 < kChunk / 256; k0 += 4) {
            f32x4 x[4], c[4], u[4], m[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t q = q0 + (size_t)(k0 + r) * 256;
                x[r] = xc[q];
                c[r] = ec[q];
                u[r] = eu[q];
                if (PREV) m[r] = mp[q];
                else m[r] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) mp[q0 + (size_t)(k0 + r) * 256] = project_add<PREV>(x[r], c[r], u[r], m[r], k, acc);
        }
    } else {
        for (size_t q = q0; q < n4; q += 256) {
            f32x4 m = {0.f, 0.f, 0.f, 0.f};
            if (PREV) m = mp[q];
            mp[q] = project_add<PREV>(xc[q], ec[q], eu[q], m, k, acc);
        }
    }
}

// The row loop of the two project updates: update_rows' shape (quads [i0, n4) of one utterance's window at a grid stride; loads x,
// c, the direction, then the solver's; stores x', its copy in the unconditional half, then the solver's) with the three-factor e
template <class LINE>
__device__ __forceinline__ void project_rows(f32x4* xc, f32x4* xu, const f32x4* ec, const f32x4* mp, LINE solver, const f32x4& f,
                                             size_t n4, size_t i0, size_t stride) {
    for (size_t i = i0; i < n4; i += stride) {
        const f32x4 xv = xc[i];
        const f32x4 c = ec[i];
        const f32x4 mv = mp[i];
        auto s = solver.load(i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ev = fmaf(f[0], xv[e], fmaf(f[1], c[e], f[2] * mv[e]));
            o[e] = solver.line(xv[e], ev, s, e);
        }
        xc[i] = o;
        xu[i] = o;
        solver.store(i, s);
    }
}

}  // namespace ditto
