// optim.hip — the fused training optimizer (gfx950; include/ditto_optim.h): AdamW with clipping by global gradient norm, an on-device
// skip of a non-finite step and an EMA of the weights, over the ~230 separate fp32 tensors a backward hands out, in three launches
// (one when neither clipping nor skipping is asked for).  Driven by a DEVICE segment table, one ditto_optim_seg per tensor; all four
// kernels run over the table's flat chunk list: chunk c = DITTO_OPTIM_CHUNK_QUADS quads of the last segment with slot0 <= c, found by
// a binary search through scalar loads (<= 16 dependent scalar reads per chunk of up to 590 KB of traffic).  A grid of
// (columns, segments) as regroup_packed_kernel's would give each of the ~200 bias and LayerNorm segments as many workgroups as the
// largest weight has chunks, nearly all of them empty; the flat list launches exactly the chunks there are.
//   optim_sqnorm_partial_kernel   chunk c: lane l reads quads l, l + 256, ... of the chunk (16-byte loads, 4 in flight), element e of a
//       quad goes into fp64 accumulator e (fma), the four meet as (a0 + a1) + (a2 + a3); the 64 lanes in a fixed xor butterfly, the 4
//       waves in index order through LDS; one double per chunk to partial[c].  The last quad of a segment is read whole and the
//       elements past n are dropped by a select (never by arithmetic: they may hold anything).  No atomics.
//   optim_norm_finish_kernel      one workgroup: lane l adds partials l, l + 256, ... in order, the same butterfly and wave order, so
//       the sum depends on n_chunks only.  norm = sqrt(sum), clip = min(1, max_norm / (norm + 1e-6)) in fp64 rounded once to fp32
//       (clip_grad_norm_'s formula; a NaN passes through as torch's clamp passes it; exactly 1 with clipping off), skip =
//       skip_nonfinite && norm is not finite.  When the launch belongs to a step it writes the state's next slot: step + 1 and
//       beta^t * beta (fp64), or on a skip the slot as it was with skipped + 1.
//   optim_adamw_apply_kernel      reads the state through scalar loads; on a skip (uniform) every workgroup returns before its first
//       vector load.  Per element, under contract(off), fl() = one rounding fp64 -> fp32 of a workgroup-uniform value:
//           gs   = g * clip
//           pd   = p * fl(1 - lr wd)
//           m'   = fmaf(fl(beta1), m, fl(1 - beta1) * gs)
//           v'   = fmaf(fl(beta2), v, fl(1 - beta2) * (gs * gs))
//           p'   = fmaf(-fl(lr / bc1), m' / fmaf(sqrtf(v'), fl(1 / sqrt(bc2)), fl(eps)), pd)
//           ema' = fmaf(fl(1 - decay), p' - ema, ema)
//       with the IEEE division and the compiler's sqrtf (<= 1 ulp; one of each per element: the kernel moves 36 - 40 B per element and stays memory
//       bound).  16-byte loads and stores, 4 quads of each of the 5 arrays in flight per lane, no LDS, no scratch; only the 1 - 3
//       elements behind a segment's last whole quad are stored as single dwords (their quad is read whole).  Without the norm launches
//       every workgroup advances step and beta^t for itself from the slot of this phase, and lane 0 of workgroup 0 writes the next
//       slot — which no workgroup of this launch reads.
//   optim_swap_kernel             p <-> ema, bit for bit, over the segments that have an ema.
#include <math.h>

#include "../../include/ditto_optim.h"
#include "common.h"
#include "model.h"

namespace ditto {

constexpr unsigned kOptChunk = DITTO_OPTIM_CHUNK_QUADS;
static_assert(kOptChunk % 1024 == 0, "a chunk is whole rounds of 4 quads per lane of 256 lanes");
static_assert(sizeof(ditto_optim_seg) == 72 && sizeof(ditto_optim_state) == 128 && sizeof(ditto_optim_slot) == 32, "documented layouts");

struct OptimArgs {
    const ditto_optim_seg* table;
    ditto_optim_state* state;
    double* partial;
    double beta1, beta2, max_norm;
    float b1, omb1, b2, omb2, eps, omd;
    int n_seg;
    unsigned n_chunks;
    int skip_nonfinite, phase, normed, advance;
};

// The tensors' addresses come out of the device table, where the compiler cannot see that they are global memory: say so, or every
// access is a flat_ instruction (which also counts against the LDS counter).
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) float gf32;
DITTO_DEV gf32x4* optim_g4(const float* p) { return (gf32x4*)(uintptr_t)p; }
DITTO_DEV gf32* optim_g1(const float* p) { return (gf32*)(uintptr_t)p; }

// The table is read-only for the whole launch: read as constant memory its entries come in through scalar loads even behind the
// kernel's own stores.
typedef const __attribute__((address_space(4))) ditto_optim_seg cseg;
DITTO_DEV cseg* optim_table(const ditto_optim_seg* t) { return (cseg*)(uintptr_t)t; }

DITTO_DEV ditto_optim_seg optim_seg_at(cseg* t, int s) {      // field by field: a struct does not copy across address spaces
    ditto_optim_seg r;
    r.p = t[s].p, r.g = t[s].g, r.m = t[s].m, r.v = t[s].v, r.ema = t[s].ema;
    r.n = t[s].n, r.slot0 = t[s].slot0, r.reserved = 0, r.lr = t[s].lr, r.weight_decay = t[s].weight_decay;
    return r;
}

// the last segment whose slot0 <= c (uniform: scalar loads)
DITTO_DEV int optim_find(cseg* t, int n_seg, unsigned c) {
    int lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t[mid].slot0 <= c) lo = mid; else hi = mid;
    }
    return lo;
}

DITTO_DEV void optim_sq_add(const f32x4& x, double (&acc)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double d = (double)x[e];
        acc[e] = fma(d, d, acc[e]);
    }
}

DITTO_DEV double optim_butterfly(double a) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m, 64);
    return a;
}

__global__ __launch_bounds__(256) void optim_sqnorm_partial_kernel(const ditto_optim_seg* __restrict__ table_, int n_seg,
                                                                   unsigned n_chunks, double* __restrict__ partial) {
    __shared__ double red[4];
    const int wave = threadIdx.x >> 6;
    cseg* table = optim_table(table_);
    for (unsigned c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int s = optim_find(table, n_seg, c);
        const uint64_t n = table[s].n;
        const gf32x4* g = optim_g4(table[s].g);
        const uint64_t q0 = (uint64_t)(c - table[s].slot0) * kOptChunk;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if ((q0 + kOptChunk) * 4 <= n) {                        // a whole chunk: 4 loads in flight per lane
#pragma unroll 1
            for (unsigned k0 = 0; k0 < kOptChunk / 256; k0 += 4) {
                f32x4 x[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = g[q0 + threadIdx.x + (uint64_t)(k0 + k) * 256];
#pragma unroll
                for (int k = 0; k < 4; ++k) optim_sq_add(x[k], acc);
            }
        } else {                                                // the segment's last chunk: the same order, as far as it goes
            for (uint64_t q = q0 + threadIdx.x; q * 4 < n && q < q0 + kOptChunk; q += 256) {
                f32x4 x = g[q];
                const uint64_t rem = n - q * 4;
#pragma unroll
                for (int e = 1; e < 4; ++e) x[e] = (uint64_t)e < rem ? x[e] : 0.f;
                optim_sq_add(x, acc);
            }
        }
        const double t = optim_butterfly((acc[0] + acc[1]) + (acc[2] + acc[3]));
        if ((threadIdx.x & 63) == 0) red[wave] = t;
        __syncthreads();
        if (threadIdx.x == 0) partial[c] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();                                        // red is written again by the next chunk of this workgroup
    }
}

__global__ __launch_bounds__(256) void optim_norm_finish_kernel(OptimArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    double acc = 0.0;
    for (unsigned j = threadIdx.x; j < a.n_chunks; j += 256) acc += a.partial[j];   // an order that depends on n_chunks only
    acc = optim_butterfly(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double norm = sqrt(((red[0] + red[1]) + red[2]) + red[3]);
    const bool finite = norm - norm == 0.0;
    double clip = 1.0;
    if (a.max_norm > 0.0) {
        const double c = a.max_norm / (norm + 1e-6);
        clip = c < 1.0 ? c : (c != c ? c : 1.0);
    }
    const int skip = a.skip_nonfinite && !finite;
    ditto_optim_state* st = a.state;
    st->norm = norm;
    st->norm32 = (float)norm;
    st->clip = (float)clip;
    st->skip = skip;
    if (a.advance) {
        const ditto_optim_slot cur = st->slot[a.phase & 1];
        ditto_optim_slot nxt = cur;
        if (skip) {
            nxt.skipped = cur.skipped + 1;
        } else {
            nxt.beta1_pow = cur.beta1_pow * a.beta1;
            nxt.beta2_pow = cur.beta2_pow * a.beta2;
            nxt.step = cur.step + 1;
        }
        st->slot[(a.phase + 1) & 1] = nxt;
    }
}

// what one chunk's elements share
struct OptimK { float clip, dk, b1, omb1, b2, omb2, rs2, eps, nss, omd; };

template <bool EMA>
DITTO_DEV void optim_elem(float& p, float g, float& m, float& v, float& ema, const OptimK& k) {
#pragma clang fp contract(off)      // the expression of the header comment, as written
    const float gs = g * k.clip;
    const float pd = p * k.dk;
    const float mn = __builtin_fmaf(k.b1, m, k.omb1 * gs);
    const float vn = __builtin_fmaf(k.b2, v, k.omb2 * (gs * gs));
    const float den = __builtin_fmaf(__builtin_sqrtf(vn), k.rs2, k.eps);
    const float pn = __builtin_fmaf(k.nss, mn / den, pd);
    if (EMA) ema = __builtin_fmaf(k.omd, pn - ema, ema);
    p = pn, m = mn, v = vn;
}

template <bool EMA>
DITTO_DEV void optim_quad(f32x4& p, const f32x4& g, f32x4& m, f32x4& v, f32x4& ema, const OptimK& k) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e], ee = ema[e];
        optim_elem<EMA>(pe, g[e], me, ve, ee, k);
        p[e] = pe, m[e] = me, v[e] = ve, ema[e] = ee;
    }
}

template <bool EMA>
DITTO_DEV void optim_apply_chunk(const ditto_optim_seg& sg, uint64_t q0, const OptimK& k) {
    const uint64_t n = sg.n;
    gf32x4* p4 = optim_g4(sg.p);
    const gf32x4* g4 = optim_g4(sg.g);
    gf32x4* m4 = optim_g4(sg.m);
    gf32x4* v4 = optim_g4(sg.v);
    gf32x4* e4 = optim_g4(sg.ema);
    gf32 *p1 = optim_g1(sg.p), *m1 = optim_g1(sg.m), *v1 = optim_g1(sg.v), *e1 = optim_g1(sg.ema);
    if ((q0 + kOptChunk) * 4 <= n) {
#pragma unroll 1
        for (unsigned k0 = 0; k0 < kOptChunk / 256; k0 += 4) {
            f32x4 p[4], g[4], m[4], v[4], e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t q = q0 + threadIdx.x + (uint64_t)(k0 + j) * 256;
                p[j] = p4[q], g[j] = g4[q], m[j] = m4[q], v[j] = v4[q];
                if (EMA) e[j] = e4[q];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t q = q0 + threadIdx.x + (uint64_t)(k0 + j) * 256;
                optim_quad<EMA>(p[j], g[j], m[j], v[j], e[j], k);
                p4[q] = p[j], m4[q] = m[j], v4[q] = v[j];
                if (EMA) e4[q] = e[j];
            }
        }
        return;
    }
    for (uint64_t q = q0 + threadIdx.x; q * 4 < n && q < q0 + kOptChunk; q += 256) {
        f32x4 p = p4[q], m = m4[q], v = v4[q], e = f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 g = g4[q];
        if (EMA) e = e4[q];
        optim_quad<EMA>(p, g, m, v, e, k);
        const uint64_t rem = n - q * 4;
        if (rem >= 4) {
            p4[q] = p, m4[q] = m, v4[q] = v;
            if (EMA) e4[q] = e;
        } else {                                                // the 1 - 3 elements behind the last whole quad
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if ((uint64_t)j < rem) {
                    p1[q * 4 + j] = p[j], m1[q * 4 + j] = m[j], v1[q * 4 + j] = v[j];
                    if (EMA) e1[q * 4 + j] = e[j];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void optim_adamw_apply_kernel(OptimArgs a) {
    const ditto_optim_state* st = a.state;
    OptimK k;
    double b1p, b2p;
    if (a.normed) {
        if (st->skip) return;                                   // uniform, before any vector load: a skipped step writes nothing
        const ditto_optim_slot sl = st->slot[(a.phase + 1) & 1];   // the finish launch has advanced it
        b1p = sl.beta1_pow, b2p = sl.beta2_pow;
        k.clip = st->clip;
    } else {
        const ditto_optim_slot sl = st->slot[a.phase & 1];
        b1p = sl.beta1_pow * a.beta1, b2p = sl.beta2_pow * a.beta2;
        k.clip = 1.f;
        if (blockIdx.x == 0 && threadIdx.x == 0) {              // the next slot: read by no workgroup of this launch
            ditto_optim_state* w = a.state;
            w->slot[(a.phase + 1) & 1] = ditto_optim_slot{b1p, b2p, sl.step + 1, sl.skipped};
            w->clip = 1.f;
            w->skip = 0;
        }
    }
    const double bc1 = 1.0 - b1p, bc2 = 1.0 - b2p;
    k.rs2 = (float)(1.0 / sqrt(bc2));
    k.b1 = a.b1, k.omb1 = a.omb1, k.b2 = a.b2, k.omb2 = a.omb2, k.eps = a.eps, k.omd = a.omd;
    cseg* table = optim_table(a.table);
    for (unsigned c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const ditto_optim_seg sg = optim_seg_at(table, optim_find(table, a.n_seg, c));
        k.dk = (float)(1.0 - sg.lr * sg.weight_decay);
        k.nss = -(float)(sg.lr / bc1);
        const uint64_t q0 = (uint64_t)(c - sg.slot0) * kOptChunk;
        if (sg.ema) optim_apply_chunk<true>(sg, q0, k); else optim_apply_chunk<false>(sg, q0, k);
    }
}

__global__ __launch_bounds__(256) void optim_swap_kernel(const ditto_optim_seg* __restrict__ table_, int n_seg, unsigned n_chunks) {
    cseg* table = optim_table(table_);
    for (unsigned c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ditto_optim_seg sg = optim_seg_at(table, optim_find(table, n_seg, c));
        if (!sg.ema) continue;
        gf32x4* p4 = optim_g4(sg.p);
        gf32x4* e4 = optim_g4(sg.ema);
        gf32 *p1 = optim_g1(sg.p), *e1 = optim_g1(sg.ema);
        const uint64_t q0 = (uint64_t)(c - sg.slot0) * kOptChunk;
        if ((q0 + kOptChunk) * 4 <= sg.n) {
#pragma unroll 1
            for (unsigned k0 = 0; k0 < kOptChunk / 256; k0 += 4) {
                f32x4 p[4], e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t q = q0 + threadIdx.x + (uint64_t)(k0 + j) * 256;
                    p[j] = p4[q], e[j] = e4[q];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t q = q0 + threadIdx.x + (uint64_t)(k0 + j) * 256;
                    p4[q] = e[j], e4[q] = p[j];
                }
            }
            continue;
        }
        for (uint64_t q = q0 + threadIdx.x; q * 4 < sg.n && q < q0 + kOptChunk; q += 256) {
            const f32x4 p = p4[q], e = e4[q];
            const uint64_t rem = sg.n - q * 4;
            if (rem >= 4) {
                p4[q] = e, e4[q] = p;
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if ((uint64_t)j < rem) p1[q * 4 + j] = e[j], e1[q * 4 + j] = p[j];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr size_t kOptMaxChunks = 0x7FFFFFFFull;
constexpr unsigned kOptMaxGrid = 1u << 20;

static unsigned optim_grid(size_t n_chunks, int grid_limit) {
    size_t g = n_chunks < kOptMaxGrid ? n_chunks : kOptMaxGrid;
    if (grid_limit > 0 && (size_t)grid_limit < g) g = (size_t)grid_limit;
    return (unsigned)g;
}

static int optim_check_table(const char* who, const void* table, int n_seg, size_t n_chunks, int grid_limit) {
    if (!table) return fail(DITTO_ERR_ARG, "%s: null table", who);
    if ((uintptr_t)table % 8) return fail(DITTO_ERR_ARG, "%s: the table must be 8-byte aligned", who);
    if (n_seg < 1 || n_seg > DITTO_OPTIM_MAX_SEGS)
        return fail(DITTO_ERR_ARG, "%s: n_seg %d outside 1 .. %d", who, n_seg, DITTO_OPTIM_MAX_SEGS);
    if (n_chunks < (size_t)n_seg || n_chunks > kOptMaxChunks)
        return fail(DITTO_ERR_ARG, "%s: n_chunks %zu outside n_seg .. 2^31 - 1 (every segment has at least one chunk)", who, n_chunks);
    if (grid_limit < 0) return fail(DITTO_ERR_ARG, "%s: grid_limit %d is negative", who, grid_limit);
    return DITTO_OK;
}

static int optim_check_hyper(const char* who, const ditto_optim_hyper* h) {
    if (!h) return fail(DITTO_ERR_ARG, "%s: null hyper", who);
    if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0))
        return fail(DITTO_ERR_ARG, "%s: betas (%g, %g) outside [0, 1)", who, h->beta1, h->beta2);
    if (!(h->eps >= 0.0) || !std::isfinite(h->eps)) return fail(DITTO_ERR_ARG, "%s: eps %g is negative or not finite", who, h->eps);
    if (!std::isfinite(h->max_norm)) return fail(DITTO_ERR_ARG, "%s: max_norm %g is not finite (<= 0 switches clipping off)", who, h->max_norm);
    if (!(h->ema_decay >= 0.0 && h->ema_decay <= 1.0)) return fail(DITTO_ERR_ARG, "%s: ema_decay %g outside [0, 1]", who, h->ema_decay);
    if ((h->skip_nonfinite != 0 && h->skip_nonfinite != 1) || h->reserved != 0)
        return fail(DITTO_ERR_ARG, "%s: skip_nonfinite must be 0 or 1 and reserved 0", who);
    return DITTO_OK;
}

static int optim_check_norm_bufs(const char* who, const void* state, const void* scratch, size_t scratch_bytes, size_t n_chunks,
                                 bool need_scratch) {
    if (!state) return fail(DITTO_ERR_ARG, "%s: null state", who);
    if ((uintptr_t)state % 16) return fail(DITTO_ERR_ARG, "%s: the state block must be 16-byte aligned", who);
    if (!need_scratch) return DITTO_OK;
    if (!scratch) return fail(DITTO_ERR_ARG, "%s: null scratch", who);
    if ((uintptr_t)scratch % 256) return fail(DITTO_ERR_ARG, "%s: the scratch must be 256-byte aligned", who);
    const size_t need = al(n_chunks * sizeof(double));
    if (scratch_bytes < need) return fail(DITTO_ERR_SIZE, "%s: scratch too small: %zu < %zu", who, scratch_bytes, need);
    return DITTO_OK;
}

static OptimArgs optim_args(const ditto_optim_seg* table, int n_seg, size_t n_chunks, const ditto_optim_hyper* h,
                            ditto_optim_state* state, void* scratch, int phase, bool normed, bool advance) {
    OptimArgs a;
    a.table = table, a.state = state, a.partial = static_cast<double*>(scratch);
    a.beta1 = h->beta1, a.beta2 = h->beta2, a.max_norm = h->max_norm;
    a.b1 = (float)h->beta1, a.omb1 = (float)(1.0 - h->beta1), a.b2 = (float)h->beta2, a.omb2 = (float)(1.0 - h->beta2);
    a.eps = (float)h->eps, a.omd = (float)(1.0 - h->ema_decay);
    a.n_seg = n_seg, a.n_chunks = (unsigned)n_chunks;
    a.skip_nonfinite = h->skip_nonfinite, a.phase = phase, a.normed = normed, a.advance = advance;
    return a;
}

static void optim_launch_norm(const OptimArgs& a, int grid_limit, hipStream_t s) {
    hipLaunchKernelGGL(optim_sqnorm_partial_kernel, dim3(optim_grid(a.n_chunks, grid_limit)), dim3(256), 0, s, a.table, a.n_seg,
                       a.n_chunks, a.partial);
    hipLaunchKernelGGL(optim_norm_finish_kernel, dim3(1), dim3(256), 0, s, a);
}

}  // namespace ditto

using namespace ditto;

extern "C" {

size_t ditto_optim_scratch_bytes(size_t n_chunks) {
    if (n_chunks < 1 || n_chunks > kOptMaxChunks) {
        fail(DITTO_ERR_ARG, "ditto_optim_scratch_bytes: n_chunks %zu outside 1 .. 2^31 - 1", n_chunks);
        return 0;
    }
    return al(n_chunks * sizeof(double));
}

int ditto_optim_grad_norm(const ditto_optim_seg* table, int n_seg, size_t n_chunks, const ditto_optim_hyper* hyper,
                          ditto_optim_state* state, void* scratch, size_t scratch_bytes, int grid_limit, ditto_stream_t stream) {
    const char* who = "ditto_optim_grad_norm";
    if (int rc = optim_check_table(who, table, n_seg, n_chunks, grid_limit)) return rc;
    if (int rc = optim_check_hyper(who, hyper)) return rc;
    if (int rc = optim_check_norm_bufs(who, state, scratch, scratch_bytes, n_chunks, true)) return rc;
    optim_launch_norm(optim_args(table, n_seg, n_chunks, hyper, state, scratch, 0, true, false), grid_limit, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return DITTO_OK;
}

int ditto_optim_adamw_step(const ditto_optim_seg* table, int n_seg, size_t n_chunks, const ditto_optim_hyper* hyper,
                           ditto_optim_state* state, int phase, void* scratch, size_t scratch_bytes, int grid_limit,
                           ditto_stream_t stream) {
    const char* who = "ditto_optim_adamw_step";
    if (int rc = optim_check_table(who, table, n_seg, n_chunks, grid_limit)) return rc;
    if (int rc = optim_check_hyper(who, hyper)) return rc;
    if (phase < 0) return fail(DITTO_ERR_ARG, "%s: phase %d is negative", who, phase);
    const bool normed = hyper->max_norm > 0.0 || hyper->skip_nonfinite;
    if (int rc = optim_check_norm_bufs(who, state, scratch, scratch_bytes, n_chunks, normed)) return rc;
    const OptimArgs a = optim_args(table, n_seg, n_chunks, hyper, state, scratch, phase, normed, true);
    if (normed) optim_launch_norm(a, grid_limit, (hipStream_t)stream);
    hipLaunchKernelGGL(optim_adamw_apply_kernel, dim3(optim_grid(n_chunks, grid_limit)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return DITTO_OK;
}

int ditto_optim_swap(const ditto_optim_seg* table, int n_seg, size_t n_chunks, int grid_limit, ditto_stream_t stream) {
    const char* who = "ditto_optim_swap";
    if (int rc = optim_check_table(who, table, n_seg, n_chunks, grid_limit)) return rc;
    hipLaunchKernelGGL(optim_swap_kernel, dim3(optim_grid(n_chunks, grid_limit)), dim3(256), 0, (hipStream_t)stream, table, n_seg,
                       (unsigned)n_chunks);
    HIP_TRY(hipGetLastError());
    return DITTO_OK;
}

}  // extern "C"
