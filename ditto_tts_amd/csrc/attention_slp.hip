// attention_slp.hip — the length predictor's attention over variable-length batches (gfx950).
//
// Two things live here, both for slp.hip's ditto_slp_forward_varlen:
//
//  1. The GEMM-composed path of attention.hip (scores fp32 -> row softmax -> P V) with per-utterance lengths.  The
//     dense path's kernels are untouched; these are their length-aware twins:
//       softmax_rows_len_kernel   a row sees min(causal rule, kv_len[b]) keys; a query row at or past q_len[b] writes
//                                 zero probabilities;
//       transpose_pad_len_kernel  V^T with ZEROS for keys at or past kv_len[b] — a probability of exactly 0 times a
//                                 NaN in a padded V row would be NaN, so the padded rows must never be multiplied.
//
//  2. Last-row attention: ONE query per (utterance, head) over keys 0 .. len_b - 1 — what the last decoder layer needs
//     when only the last position reaches length_predictor.  Memory-bound (every K and V row is read once, 16 bytes
//     per lane), no score matrix in HBM: the keys of a (utterance, head) are split into chunks of g_slp_lr_chunk keys,
//     one workgroup per chunk writes a partial (max, sum, output), a second kernel merges the partials in chunk
//     order.  No atomics: the same bits every run.  Keys at or past len_b are never loaded.
#include "common.h"
#include "kernels.h"

namespace ditto {

int g_slp_lr_chunk = 128;   // keys per workgroup of the last-row kernel (ditto_set_option("slp_lr_chunk"))
int g_slp_last_row = 1;     // ditto_slp_forward_varlen: last layer on the last rows only (0 = every layer composed)

namespace {

constexpr int LR_MAX_CHUNK = 1024;   // LDS: scores + probabilities of one chunk
constexpr int LR_MAX_DH = 2048;

DITTO_DEV int clamp_len(const int32_t* len, int b, int full) {
    if (!len) return full;
    const int v = len[b];
    return v < 1 ? 1 : (v > full ? full : v);
}

// softmax_rows_kernel with lengths.  Rows are [pair z][query i] of the chunk that starts at (batch, head) pair bh0.
__global__ __launch_bounds__(256) void softmax_rows_len_kernel(const float* __restrict__ S, bf16* __restrict__ P, int rows,
                                                               int Sq, int Skv, int ld, float scale_log2, int causal,
                                                               int H, int bh0, const int32_t* __restrict__ q_len,
                                                               const int32_t* __restrict__ kv_len) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = (bh0 + row / Sq) / H, i = row % Sq;
    const int ql = clamp_len(q_len, b, Sq), kl = clamp_len(kv_len, b, Skv);
    int vis = kl;   // number of visible keys
    if (causal) {
        vis = i + (kl - ql) + 1;   // the utterance's own mask: key j <= i + (kv_len - q_len)
        vis = vis < 0 ? 0 : (vis > kl ? kl : vis);
    }
    if (i >= ql) vis = 0;
    const float* s = S + (size_t)row * ld;
    float m = -1e30f;
    for (int j = lane; j < vis; j += 64) m = fmaxf(m, s[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < vis; j += 64) sum += __builtin_amdgcn_exp2f((s[j] - m) * scale_log2);
    sum = wave_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
    bf16* pr = P + (size_t)row * ld;
    for (int j = lane; j < ld; j += 64)
        pr[j] = j < vis ? (bf16)(__builtin_amdgcn_exp2f((s[j] - m) * scale_log2) * inv) : (bf16)0.f;
}

// transpose_pad_kernel with lengths: keys at or past kv_len[b] are written as zeros and never loaded.
__global__ __launch_bounds__(256) void transpose_pad_len_kernel(const bf16* __restrict__ V, int ldv, bf16* __restrict__ Vt,
                                                                int ldT, int Skv, int dh, int H, int bh0, long long vs_b,
                                                                long long vs_h, const int32_t* __restrict__ kv_len) {
    __shared__ bf16 tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int k0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int bh = bh0 + blockIdx.z;
    const int kl = clamp_len(kv_len, bh / H, Skv);
    V += (long long)(bh / H) * vs_b + (long long)(bh % H) * vs_h;
    Vt += (size_t)blockIdx.z * dh * ldT;
    for (int i = ty; i < 32; i += 8) {
        const int key = k0 + i, dd = d0 + tx;
        tile[i][tx] = (key < kl && dd < dh) ? V[(size_t)key * ldv + dd] : (bf16)0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int dd = d0 + i, key = k0 + tx;
        if (dd < dh && key < ldT) Vt[(size_t)dd * ldT + key] = tile[tx][i];
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t generic_fwd_bytes(int Sq, int Skv, int dh) {   // one (batch, head): attention.hip's layout
    const size_t ld = (size_t)((Skv + 63) / 64) * 64;
    return align256((size_t)Sq * ld * 4) + align256((size_t)Sq * ld * 2) + align256((size_t)dh * ld * 2);
}

// ---- last-row attention --------------------------------------------------------------------------------------------
// A head row of dh bf16 is NV = dh / 8 vectors of 16 bytes.  A wave works on KPW = 64 / G keys at once, G lanes per key
// (G = 8, 16, 32 or 64: the power of two >= min(NV, 64)); lane l of a group holds vectors l, l + G, ... (CH of them).
// The same layout serves q . k (reduced over the G lanes of a group) and p . v (accumulated per lane, the groups summed
// at the end), so K and V are both read as whole 16-byte vectors, consecutive lanes on consecutive addresses.
DITTO_DEV void load8(const bf16* p, float (&f)[8]) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = bf16_lo(u[e]);
        f[2 * e + 1] = bf16_hi(u[e]);
    }
}

// grid (chunks, H, B), 256 threads.  part_ml [B * H * NC][2] = (max of the raw scores, sum of exp2((s - max) * scale_log2)),
// part_o [B * H * NC][dh] = sum_j exp2(..) v_j, both over the chunk's keys [c * chunk, min((c + 1) * chunk, len_b)).
template <int CH>
__global__ __launch_bounds__(256) void last_row_partial_kernel(const bf16* __restrict__ Q, int ldq, const bf16* __restrict__ K,
                                                               int ldk, long long ks_b, const bf16* __restrict__ V, int ldv,
                                                               long long vs_b, const int32_t* __restrict__ len, int Skv,
                                                               int dh, int G, int chunk, float scale_log2,
                                                               float* __restrict__ part_ml, float* __restrict__ part_o) {
    __shared__ float sc[LR_MAX_CHUNK];
    __shared__ float pr[LR_MAX_CHUNK];
    __shared__ float red[4][CH * 512];
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, NC = gridDim.x, H = gridDim.y;
    const int L = clamp_len(len, b, Skv);
    const int k0 = c * chunk;
    if (k0 >= L) return;   // nothing of this utterance in the chunk: the merge never reads its slot
    const int k1 = k0 + chunk < L ? k0 + chunk : L, n = k1 - k0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int KPW = 64 / G, g = lane / G, l = lane % G, NV = dh >> 3;
    const bf16* q = Q + (size_t)b * ldq + (size_t)h * dh;
    K += (long long)b * ks_b + (size_t)h * dh;
    V += (long long)b * vs_b + (size_t)h * dh;

    float qf[CH][8];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const int vi = l + G * ch;
        if (vi < NV) load8(q + vi * 8, qf[ch]);
        else
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[ch][e] = 0.f;
    }
    // scores: wave w takes keys k0 + (it * 4 + w) * KPW + g
    for (int kb = k0; kb < k1; kb += 4 * KPW) {   // workgroup-uniform trip count: the shuffles below see whole waves
        const int key = kb + w * KPW + g;
        float acc = 0.f;
        if (key < k1) {
            const bf16* kr = K + (size_t)key * ldk;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const int vi = l + G * ch;
                if (vi < NV) {
                    float kf[8];
                    load8(kr + vi * 8, kf);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(qf[ch][e], kf[e], acc);
                }
            }
        }
        for (int off = 1; off < G; off <<= 1) acc += __shfl_xor(acc, off, 64);
        if (l == 0 && key < k1) sc[key - k0] = acc;
    }
    __syncthreads();
    float m = -__builtin_huge_valf();
    for (int j = lane; j < n; j += 64) m = fmaxf(m, sc[j]);
    m = wave_max(m);   // every wave holds the chunk's maximum
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) {
        const float p = __builtin_amdgcn_exp2f((sc[j] - m) * scale_log2);
        sum += p;
        if (w == 0) pr[j] = p;
    }
    sum = wave_sum(sum);
    __syncthreads();
    // p . v with the same key and vector assignment
    float of[CH][8];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int e = 0; e < 8; ++e) of[ch][e] = 0.f;
    for (int kb = k0; kb < k1; kb += 4 * KPW) {
        const int key = kb + w * KPW + g;
        if (key < k1) {
            const float p = pr[key - k0];
            const bf16* vr = V + (size_t)key * ldv;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const int vi = l + G * ch;
                if (vi < NV) {
                    float vf[8];
                    load8(vr + vi * 8, vf);
#pragma unroll
                    for (int e = 0; e < 8; ++e) of[ch][e] = __builtin_fmaf(p, vf[e], of[ch][e]);
                }
            }
        }
    }
    // the KPW key groups of a wave (lanes l, l + G, ...), then the four waves in order
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            for (int off = G; off < 64; off <<= 1) of[ch][e] += __shfl_xor(of[ch][e], off, 64);
    if (g == 0) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            const int vi = l + G * ch;
            if (vi < NV)
#pragma unroll
                for (int e = 0; e < 8; ++e) red[w][vi * 8 + e] = of[ch][e];
        }
    }
    __syncthreads();
    const size_t slot = ((size_t)b * H + h) * NC + c;
    float* po = part_o + slot * dh;
    for (int dd = threadIdx.x; dd < dh; dd += 256) po[dd] = ((red[0][dd] + red[1][dd]) + red[2][dd]) + red[3][dd];
    if (threadIdx.x == 0) {
        part_ml[slot * 2] = m;
        part_ml[slot * 2 + 1] = sum;
    }
}

// grid (H, B): out[b, h * dh + c] = sum_c w_c o_c / sum_c w_c sum_c, w_c = exp2((m_c - max m) * scale_log2), chunks in order
__global__ __launch_bounds__(256) void last_row_merge_kernel(const float* __restrict__ part_ml, const float* __restrict__ part_o,
                                                             const int32_t* __restrict__ len, int Skv, int dh, int chunk,
                                                             int NC, float scale_log2, bf16* __restrict__ out, int ldo) {
    const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
    const int L = clamp_len(len, b, Skv);
    const int nc = (L + chunk - 1) / chunk;
    const size_t slot0 = ((size_t)b * H + h) * NC;
    float M = -__builtin_huge_valf();
    for (int c = 0; c < nc; ++c) M = fmaxf(M, part_ml[(slot0 + c) * 2]);
    float den = 0.f;
    for (int c = 0; c < nc; ++c)
        den += __builtin_amdgcn_exp2f((part_ml[(slot0 + c) * 2] - M) * scale_log2) * part_ml[(slot0 + c) * 2 + 1];
    const float inv = 1.0f / den;
    for (int dd = threadIdx.x; dd < dh; dd += 256) {
        float o = 0.f;
        for (int c = 0; c < nc; ++c)
            o += __builtin_amdgcn_exp2f((part_ml[(slot0 + c) * 2] - M) * scale_log2) * part_o[(slot0 + c) * dh + dd];
        out[(size_t)b * ldo + (size_t)h * dh + dd] = (bf16)(o * inv);
    }
}

}  // namespace

size_t attention_last_row_workspace_bytes(int B, int H, int Skv, int dh) {
    const size_t NC = (size_t)(Skv + g_slp_lr_chunk - 1) / g_slp_lr_chunk;
    return align256((size_t)B * H * NC * 2 * 4) + align256((size_t)B * H * NC * dh * 4);
}

hipError_t launch_attention_last_row(const LastRowAttnArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.H <= 0 || a.Skv <= 0 || a.dh <= 0 || a.dh % 64 || a.dh > LR_MAX_DH) return hipErrorInvalidValue;
    if (!a.q || !a.k || !a.v || !a.out || !a.workspace) return hipErrorInvalidValue;
    // 16-byte vector loads: every row start must be 16-byte aligned
    if ((a.ldq | a.ldk | a.ldv) % 8 || (a.ks_b | a.vs_b) % 8) return hipErrorInvalidValue;
    if (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) % 16 || (uintptr_t)a.workspace % 256) return hipErrorInvalidValue;
    if (a.B > 65535 || a.H > 65535) return hipErrorInvalidValue;
    const int chunk = g_slp_lr_chunk;
    if (chunk < 1 || chunk > LR_MAX_CHUNK) return hipErrorInvalidValue;
    if (a.workspace_bytes < attention_last_row_workspace_bytes(a.B, a.H, a.Skv, a.dh)) return hipErrorInvalidValue;
    const int NC = (a.Skv + chunk - 1) / chunk;
    float* ml = (float*)a.workspace;
    float* po = (float*)((char*)a.workspace + align256((size_t)a.B * a.H * NC * 2 * 4));
    const int NV = a.dh / 8;
    int G = 8;
    while (G < 64 && G < NV) G <<= 1;
    const int CH = (NV + G - 1) / G;
    const float sl2 = a.scale * 1.4426950408889634f;
    const dim3 grid(NC, a.H, a.B), block(256);
#define DITTO_LR(C)                                                                                                    \
    case C:                                                                                                            \
        hipLaunchKernelGGL((last_row_partial_kernel<C>), grid, block, 0, s, (const bf16*)a.q, a.ldq, (const bf16*)a.k, \
                           a.ldk, a.ks_b, (const bf16*)a.v, a.ldv, a.vs_b, a.len, a.Skv, a.dh, G, chunk, sl2, ml, po); \
        break;
    switch (CH) {
        DITTO_LR(1) DITTO_LR(2) DITTO_LR(3) DITTO_LR(4)
        default: return hipErrorInvalidValue;
    }
#undef DITTO_LR
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(last_row_merge_kernel, dim3(a.H, a.B), block, 0, s, ml, po, a.len, a.Skv, a.dh, chunk, NC, sl2,
                       (bf16*)a.out, a.ldo);
    return hipGetLastError();
}

// attention.hip's GEMM-composed path with lengths (a.q_len / a.kv_len, either may be null); bf16 output only, no dropout.
hipError_t launch_attention_composed_len(const AttnArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.H <= 0 || a.Sq <= 0 || a.Skv <= 0 || a.dh <= 0 || a.dh % 64) return hipErrorInvalidValue;
    if (a.resid_f32 || a.dropout_p > 0.f || a.lse_out || a.cu_q || a.cu_kv || !a.out_bf16) return hipErrorInvalidValue;
    const float LOG2E = 1.4426950408889634f;
    const int ld = ((a.Skv + 63) / 64) * 64;
    const int BH = a.B * a.H;
    const size_t one = generic_fwd_bytes(a.Sq, a.Skv, a.dh);
    if (!a.workspace || a.workspace_bytes < one) return hipErrorInvalidValue;
    int chunk = (int)(a.workspace_bytes / one < (size_t)BH ? a.workspace_bytes / one : (size_t)BH);
    // only batch chunks that are whole runs of heads / batches: either all H heads of some batches, or heads of one batch
    if (chunk >= a.H) chunk = (chunk / a.H) * a.H;
    else while (a.H % chunk) --chunk;
    char* ws = (char*)a.workspace;
    const size_t sS = (size_t)a.Sq * ld, sV = (size_t)a.dh * ld;
    float* S = (float*)ws;
    bf16* P = (bf16*)(ws + align256((size_t)chunk * sS * 4));
    bf16* Vt = (bf16*)((char*)P + align256((size_t)chunk * sS * 2));
    for (int bh0 = 0; bh0 < BH; bh0 += chunk) {
        const int nb = chunk < BH - bh0 ? chunk : BH - bh0;
        const int b0 = bh0 / a.H, h0 = bh0 % a.H;
        const int nz_o = nb >= a.H ? nb / a.H : 1, nz_i = nb >= a.H ? a.H : nb;
        const bf16* q = (const bf16*)a.q + (size_t)b0 * a.Sq * a.ldq + h0 * a.dh;
        const bf16* k = (const bf16*)a.k + (size_t)b0 * a.Skv * a.ldk + h0 * a.dh;
        GemmArgs g1{};
        g1.A = q; g1.lda = a.ldq; g1.W = k; g1.ldw = a.ldk; g1.out = S; g1.ldo = ld;
        g1.M = a.Sq; g1.N = ld; g1.K = a.dh; g1.w_rows = a.Skv;
        g1.batch_outer = nz_o; g1.batch_inner = nz_i;
        g1.sA[0] = (long long)a.Sq * a.ldq; g1.sA[1] = a.dh; g1.sW[0] = (long long)a.Skv * a.ldk; g1.sW[1] = a.dh;
        g1.sO[0] = (long long)nz_i * sS; g1.sO[1] = (long long)sS;
        hipError_t e = launch_gemm(g1, EPI_BIAS_F32, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(softmax_rows_len_kernel, dim3((nb * a.Sq + 3) / 4), dim3(256), 0, s, S, P, nb * a.Sq, a.Sq, a.Skv,
                           ld, a.scale * LOG2E, a.causal ? 1 : 0, a.H, bh0, a.q_len, a.kv_len);
        hipLaunchKernelGGL(transpose_pad_len_kernel, dim3(ld / 32, (a.dh + 31) / 32, nb), dim3(256), 0, s, (const bf16*)a.v,
                           a.ldv, Vt, ld, a.Skv, a.dh, a.H, bh0, (long long)a.Skv * a.ldv, (long long)a.dh, a.kv_len);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        GemmArgs g2{};
        g2.A = P; g2.lda = ld; g2.W = Vt; g2.ldw = ld; g2.M = a.Sq; g2.N = a.dh; g2.K = ld; g2.w_rows = a.dh;
        g2.batch_outer = nz_o; g2.batch_inner = nz_i;
        g2.sA[0] = (long long)nz_i * sS; g2.sA[1] = (long long)sS; g2.sW[0] = (long long)nz_i * sV; g2.sW[1] = (long long)sV;
        g2.out = (bf16*)a.out_bf16 + (size_t)b0 * a.Sq * a.ldo + h0 * a.dh; g2.ldo = a.ldo;
        g2.sO[0] = (long long)a.Sq * a.ldo; g2.sO[1] = a.dh;
        e = launch_gemm(g2, EPI_BIAS_BF16, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace ditto
