// guided_update.h — the one source of the fused guided (DDIM) update of guided.hip and guided_packed.hip, and of the spans of every
// packed update, multistep and span-training kernel.
//   e' = CFG ? fmaf(w[b], c - u, u) : c               c, u = the conditional / unconditional half of eps2 (cfg_combine_kernel's expression)
//   x' = fmaf(a[b], x, fmaf(ce[b], e', cz[b] * z))    (linear_update_kernel's; z = cz = 0 without noise)
// written to the conditional and, under CFG, the unconditional half of x2.  NOISE: 0 none, 1 a buffer laid out like x, 2 Philox of
// (seeds[b], step, quad index inside the utterance) — ditto_noise_normal's bits (philox.h).  HBM-bound: per element CFG 4 reads (x,
// c, u, buffer noise) + 2 writes, without CFG 3 + 1; 16-byte lane accesses, grid (chunks, B); d % 64 == 0: no quad straddles a row.
#pragma once
#include <type_traits>
#include "common.h"
#include "philox.h"

namespace ditto {

// what utterance b multiplies with (s_loads: b = blockIdx.y is uniform over the workgroup)
struct GuidedCoef { float a, ce, cz, w; unsigned long long seed; };
template <int NOISE, bool CFG>
__device__ __forceinline__ GuidedCoef guided_coef(const float* a, const float* ce, const float* cz, const float* w,
                                                  const int64_t* seeds, int b) {
    return {a[b], ce[b], NOISE ? cz[b] : 0.f, CFG ? w[b] : 0.f, NOISE == 2 ? (unsigned long long)seeds[b] : 0ull};
}

// utterance b's rows [cu[b], cu[b+1]) of a packed [S, d] buffer, clamped like attn_span: r0 into [0, S - 1], nb into [1, S - r0] (never
// outside the S rows, at least one row)
struct UttRows { int r0, nb; };
__device__ __forceinline__ UttRows utt_rows(const int32_t* cu, int b, int S) {
    int r0 = cu[b];
    r0 = r0 < 0 ? 0 : (r0 > S - 1 ? S - 1 : r0);
    const int n = cu[b + 1] - r0, nb = n < 1 ? 1 : (n > S - r0 ? S - r0 : n);
    return {r0, nb};
}

// The one span of the packed update, multistep and span-training kernels: utterance b with a clean speech PROMPT of prompt_len[b] rows
// in front and a clean SUFFIX of suffix_len[b] rows behind (speech infilling); the rows in between, [cu[b] + P_b, cu[b+1] - Q_b), are
// the generated window: g4 quads from quad p4 on, of the utterance's n4 from quad base4 on.  Either pointer may be NULL: 0 rows.  P_b
// is clamped into [0, n_b - 1], then Q_b into [0, n_b - 1 - P_b]: at least one row is generated, and a bad value gives wrong rows, never
// an access outside the utterance's own.  b = blockIdx.y is uniform over the workgroup, so cu, P_b and Q_b come in through scalar loads
// and the NULL tests are scalar branches.
//
// P and Q are run-time values and TAGS is a template parameter, for one reason each.  A NULL length and a length of 0 give the same
// span, so one kernel serves the unprompted, prompted and windowed entries bit for bit, at two scalar loads per workgroup.  The
// per-utterance tag form is not such a special case of the scalar one: it skips the Philox draw of an utterance whose cz is 0 and adds
// cz * 0 = +0 where the scalar form adds cz * z = 0 * z, a zero of z's sign, and fmaf carries that sign into a result that is itself 0.
// So the two forms differ in bits and stay two instantiations.
struct WindowSpan { size_t base4, n4, p4, g4; };
__device__ __forceinline__ WindowSpan window_span(const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int b, int S,
                                                  int d) {
    const UttRows u = utt_rows(cu, b, S);
    int p = prompt_len ? prompt_len[b] : 0;
    p = p < 0 ? 0 : (p > u.nb - 1 ? u.nb - 1 : p);
    int q = suffix_len ? suffix_len[b] : 0;
    q = q < 0 ? 0 : (q > u.nb - 1 - p ? u.nb - 1 - p : q);
    return {(size_t)u.r0 * d / 4, (size_t)u.nb * d / 4, (size_t)p * d / 4, (size_t)(u.nb - p - q) * d / 4};
}

// the generated rows of utterance b without a suffix, [cu[b] + P_b, cu[b+1]) (prompt_len NULL: the whole utterance): what the
// guidance-rescale statistics run over (guided_rescale.hip, which is held to its machine code: window_span's g4 is another expression)
struct GuidedSpan { size_t base4, n4; };
__device__ __forceinline__ GuidedSpan generated_span(const int32_t* cu, const int32_t* prompt_len, int b, int S, int d) {
    if (prompt_len) {
        const UttRows u = utt_rows(cu, b, S);
        int p = prompt_len[b];
        p = p < 0 ? 0 : (p > u.nb - 1 ? u.nb - 1 : p);
        const size_t base4 = (size_t)u.r0 * d / 4, n4 = (size_t)u.nb * d / 4, p4 = (size_t)p * d / 4;
        return {base4 + p4, n4 - p4};
    }
    const UttRows u = utt_rows(cu, b, S);
    return {(size_t)u.r0 * d / 4, (size_t)u.nb * d / 4};
}

// utterance b of a step in which G of the B utterances are guided (guided_mixed.hip): its generated rows and, with a partner, the
// same rows of its unconditional copy behind row S.  Clamps: utt_rows' and window_span's of P_b; the partner into [-1, G - 1]; the copy's
// span has b's own length n_b, its first row clamped into [S, S + S_G - n_b] (no copy at all when n_b > S_G: g = -1).  The offset
// cu[B + g + 1] is not read.  Statement for statement the head of guided_update_mixed_kernel, which keeps its own text: routed through
// this helper its scalar instructions come out in another order, and that kernel is held to its machine code
// (tests/test_gpu_rescale_kernel.py holds these clamps to the values documented for that kernel).
struct MixedSpan { size_t base4, n4; int urow, g; };     // urow: the copy's first generated row (g >= 0 only)
__device__ __forceinline__ MixedSpan mixed_span(const int32_t* cu, const int32_t* partner, const int32_t* prompt_len, int b, int B,
                                                int G, int S, int S_G, int d) {
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
    p = p < 0 ? 0 : (p > n - 1 ? n - 1 : p);                        // window_span's clamp of P_b
    const size_t d4 = (size_t)d / 4;
    return {(size_t)(r0 + p) * d4, (size_t)(n - p) * d4, u0 + p, g};
}

// quads [i0, n4) of one utterance at a grid stride: xc / ec (xu / eu) = its first quad in the conditional (unconditional) half, nz in
// the noise buffer.  PADDED: quads from valid4 on are written as 0 and read nothing.  draw: whether a Philox utterance draws at all.
// i0 and stride come from the __global__ function: read here, blockDim / gridDim compile to a vector load of the implicit arguments.
template <int NOISE, bool CFG, bool PADDED>
__device__ __forceinline__ void guided_rows(f32x4* xc, f32x4* xu, const f32x4* ec, const f32x4* eu, const f32x4* nz,
                                            const GuidedCoef& k, unsigned step, bool draw, size_t n4, size_t valid4, size_t i0,
                                            size_t stride) {
    for (size_t i = i0; i < n4; i += stride) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (!PADDED || i < valid4) {
            const f32x4 xv = xc[i];
            const f32x4 c = ec[i];
            f32x4 u = c;
            if (CFG) u = eu[i];
            f32x4 zv = {0.f, 0.f, 0.f, 0.f};
            if (NOISE == 1) zv = nz[i];
            if (NOISE == 2 && draw) zv = normal4(k.seed, step, i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ev = CFG ? fmaf(k.w, c[e] - u[e], u[e]) : c[e];
                o[e] = fmaf(k.a, xv[e], fmaf(k.ce, ev, k.cz * zv[e]));
            }
        }
        xc[i] = o;
        if (CFG) xu[i] = o;
    }
}

// 256-thread workgroups over the quads of the longest utterance (at most 1024: the kernels stride), one grid column per utterance
inline dim3 guided_grid(int max_rows, int d, int B) {
    const size_t n4 = (size_t)max_rows * d / 4;
    size_t gx = (n4 + 255) / 256;
    if (gx > 1024) gx = 1024;
    return dim3((unsigned)gx, B);
}

// f(noise mode, CFG) with both as compile-time constants: the six instantiations of a kernel
template <class F> inline hipError_t guided_dispatch(const float* noise, const int64_t* seeds, bool cfg, F&& f) {
    auto g = [&](auto nz) { return cfg ? f(nz, std::true_type{}) : f(nz, std::false_type{}); };
    return seeds ? g(std::integral_constant<int, 2>{}) : noise ? g(std::integral_constant<int, 1>{}) : g(std::integral_constant<int, 0>{});
}

}  // namespace ditto
