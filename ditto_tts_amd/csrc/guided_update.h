// guided_update.h — the one source of every fused sampling update: the row loop (update_rows) that guided.hip, guided_packed.hip,
// guided_multistep.hip, guided_mixed.hip, guided_refresh.hip and guided_reuse.hip's multistep kernel all run (guided_reuse.hip's DDIM
// kernel alone keeps a written-out copy and says why), and the spans of every packed update,
// multistep and span-training kernel.  The loop is one piece of arithmetic in two parts, each a compile-time choice:
//   e' = c | fmaf(w[b], c - u, u) | the same with c - u kept | fmaf(w[b] - 1, kept, c)      (the EPS_ modes; cfg_combine_kernel's
//                                                      expression; c, u = the conditional / unconditional prediction)
//   x' = fmaf(a[b], x, fmaf(ce[b], e', cz[b] * z))    (DdimLine: linear_update_kernel's; z = cz = 0 without noise)
//      | fmaf(a, x, fmaf(b, x0, g q)), x0 = fmaf(kx, x, ke e'), q = x0                      (MultistepLine)
// written to the conditional and, where there is one, the unconditional half of x2.  The kernels stay separate launches with their
// own spans, coefficients and branches; what they share is this text, so the bit equalities the tests hold between them (STORE = the
// CFG form, a refresh row = the mixed kernel's, a reuse row = the LOAD line) hold by construction.
// NOISE: 0 none, 1 a buffer laid out like x, 2 Philox of
// (seeds[b], step, quad index inside the utterance) — ditto_noise_normal's bits (philox.h).  HBM-bound: per element CFG 4 reads (x,
// c, u, buffer noise) + 2 writes, without CFG 3 + 1; 16-byte lane accesses, grid (chunks, B); d % 64 == 0: no quad straddles a row.
#pragma once
#include <type_traits>
#include "common.h"
#include "ditto_hip.h"
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
// guidance-rescale statistics run over.  The same span as window_span's with a NULL suffix, and guided_rescale.hip is held to its
// machine code: with window_span there (base4 + p4, g4) its partial kernel came out at 631 instructions for 643 and its finish kernel
// at 445 for 449 — g4 = (n - p) d / 4 is another expression than n4 - p4, and the NULL test of the suffix stays — so this stays
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
// cu[B + g + 1] is not read.  Statement for statement the head of guided_update_mixed_kernel, which keeps its own text: that kernel
// is held to its machine code, and called from there this helper gives all three instantiations the same instruction count with
// the two scalar adds of S + S_G - n moved in front of the load of cu[B + g] and its wait
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

// How the guided prediction e of a quad comes about
enum {
    EPS_COND = 0,    // e = c: the conditional prediction alone
    EPS_CFG = 1,     // e = fmaf(w, c - u, u)
    EPS_STORE = 2,   // dl = c - u, e = fmaf(w, dl, u): EPS_CFG's bits, and dl is written to the direction buffer
    EPS_LOAD = 3     // e = fmaf(w - 1.0f, dl, c): dl is read from the direction buffer and never written
};

// The solver line that follows e, as a policy of update_rows: what it loads per quad (load), the result of one element (line, which
// leaves what is to be stored in element j of the loaded quad) and what it stores per quad (store).
// The DDIM line: z from a buffer (nz = the utterance's first quad in it) or Philox; draw: whether a Philox utterance draws at all
template <int NOISE> struct DdimLine {
    const f32x4* nz; const GuidedCoef& k; unsigned step; bool draw;
    __device__ __forceinline__ f32x4 load(size_t i) const {
        f32x4 zv = {0.f, 0.f, 0.f, 0.f};
        if (NOISE == 1) zv = nz[i];
        if (NOISE == 2 && draw) zv = normal4(k.seed, step, i);
        return zv;
    }
    __device__ __forceinline__ float line(float x, float e, f32x4& z, int j) const { return fmaf(k.a, x, fmaf(k.ce, e, k.cz * z[j])); }
    __device__ __forceinline__ void store(size_t, const f32x4&) const {}
};
// The multistep (DPM-Solver++(2M)) lines: qp = the utterance's first quad of the x0 history.  PREV false: q is written and never
// read — the first step of an utterance meets an uninitialised history
template <bool PREV> struct MultistepLine {
    f32x4* qp; const ::ditto_multistep_coef& k;
    __device__ __forceinline__ f32x4 load(size_t i) const {
        f32x4 qv = {0.f, 0.f, 0.f, 0.f};
        if (PREV) qv = qp[i];
        return qv;
    }
    __device__ __forceinline__ float line(float x, float e, f32x4& q, int j) const {
        const float x0 = fmaf(k.kx, x, k.ke * e);
        const float o = fmaf(k.a, x, fmaf(k.b, x0, PREV ? k.g * q[j] : 0.f));
        q[j] = x0;
        return o;
    }
    __device__ __forceinline__ void store(size_t i, const f32x4& q) const { qp[i] = q; }
};

// The row loop of the fused updates: quads [i0, n4) of one utterance's generated rows at a grid stride.  xc / ec (xu / eu) = its
// first quad in the conditional (unconditional) half, dp in the direction buffer.  Per quad the loads are x, c, then u or the
// direction, then the solver's; the stores x', its copy in the unconditional half (EPS_CFG and EPS_STORE always, EPS_LOAD with the
// run-time `mirror`, EPS_COND never), then the solver's, then the direction.  PADDED: quads from valid4 on are written as 0 and read
// nothing.  i0 and stride come from the __global__ function: read here, blockDim / gridDim compile to a vector load of the implicit
// arguments.  The solver is passed by value and stands between eu and dp: with a reference, or behind mirror, the scalar code of
// several kernels comes out in another order than the loops this one replaced (tools/asm_identity.py).
template <int MODE, bool PADDED, class LINE>
__device__ __forceinline__ void update_rows(f32x4* xc, f32x4* xu, const f32x4* ec, const f32x4* eu, LINE solver, f32x4* dp, float w,
                                            bool mirror, size_t n4, size_t valid4, size_t i0, size_t stride) {
    static_assert(!PADDED || MODE == EPS_COND || MODE == EPS_CFG, "only guided.hip's two plain modes know padding rows");
    const float wm1 = w - 1.0f;
    for (size_t i = i0; i < n4; i += stride) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f}, s, dl;
        if (!PADDED || i < valid4) {
            const f32x4 xv = xc[i];
            const f32x4 c = ec[i];
            f32x4 u = c;
            if (MODE == EPS_CFG || MODE == EPS_STORE) u = eu[i];
            if (MODE == EPS_LOAD) dl = dp[i];
            s = solver.load(i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (MODE == EPS_CFG || MODE == EPS_STORE) dl[e] = c[e] - u[e];
                const float ev = MODE == EPS_COND ? c[e] : MODE == EPS_LOAD ? fmaf(wm1, dl[e], c[e]) : fmaf(w, dl[e], u[e]);
                o[e] = solver.line(xv[e], ev, s, e);
            }
        }
        xc[i] = o;
        if (MODE == EPS_CFG || MODE == EPS_STORE || (MODE == EPS_LOAD && mirror)) xu[i] = o;
        solver.store(i, s);
        if (MODE == EPS_STORE) dp[i] = dl;
    }
}

// 256-thread workgroups over the quads of the longest utterance (at most 1024: the kernels stride), one grid column per utterance
inline dim3 guided_grid(int max_rows, int d, int B) {
    const size_t n4 = (size_t)max_rows * d / 4;
    size_t gx = (n4 + 255) / 256;
    if (gx > 1024) gx = 1024;
    return dim3((unsigned)gx, B);
}

// f(noise mode) with the mode as a compile-time constant: 2 Philox (seeds), 1 a buffer (noise), 0 none — the one place that says so;
// and f(noise mode, CFG) on top of it: the six instantiations of a kernel
template <class F> inline auto noise_dispatch(const float* noise, const int64_t* seeds, F&& f) {
    return seeds ? f(std::integral_constant<int, 2>{}) : noise ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}
template <class F> inline hipError_t guided_dispatch(const float* noise, const int64_t* seeds, bool cfg, F&& f) {
    return noise_dispatch(noise, seeds, [&](auto nz) { return cfg ? f(nz, std::true_type{}) : f(nz, std::false_type{}); });
}

}  // namespace ditto
