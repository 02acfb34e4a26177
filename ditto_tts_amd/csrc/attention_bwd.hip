// attention_bwd.hip — fused (flash-style) attention BACKWARD for gfx950, head_dim 64, bf16 in / fp32 accumulate.
//
// Backward of  O = dropout(softmax(q k^T * scale)) v  (self-attention, reference src/components/DiT.py:131-134, and
// nn.MultiheadAttention's cross-attention, :144-148, dropout 0.1 in train mode) with the probabilities RECOMPUTED
// from q, k and the forward's log-sum-exp, never stored:
//     P = exp2(c s - L),   dP = mask/(1-p) * (dO v^T),   dS = P * (dP - delta) * scale,   delta = rowsum(dO * O)
//     dV = (mask/(1-p) * P)^T dO,    dQ = dS k,    dK = dS^T q.
// Two kernels, so that every output is owned by exactly one workgroup: NO atomics and no cross-workgroup sum =>
// bit-reproducible gradients.
//   dq kernel    one workgroup = 128 queries; streams 64-key tiles.   S^T = K Q^T and dP^T = V dO^T have the QUERY
//                on the lane (L and delta are per-lane scalars; the query fragments carry scale * log2(e) and the score
//                chain starts from -L, as in the training forward); dS^T, packed to bf16 in registers, is the B operand
//                of dQ^T += K^T dS^T (K^T by ds_read_b64_tr_b16 from the same LDS image the row reads use).
//   dkdv kernel  one workgroup = 128 keys; streams 64-query tiles.   S = Q K^T and dP = dO V^T have the KEY on the
//                lane (K, V fragments live in registers for the whole kernel); P and dS in registers are the B
//                operands of dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T by transposed reads).
// This costs 7 products instead of the 5 of a single-kernel backward (S and dP are computed in both), 14 B H Sq Skv
// dh FLOPs per call: 40 % more MFMA work bought for determinism and for not needing fp32 dQ atomics.
// Roofline: nominally MFMA (K/V or Q/dO of one head are re-read from the XCD's L2), in practice vector ISSUE: a 64-row
// tile carries as many cycles of P / dS arithmetic as of MFMA (see the comment above the kernel and profiles/r03_attn_bwd.txt).
#include <type_traits>

#include "gemm_common.h"

namespace ditto {

namespace {

#include "attn64bwd.h"

}  // namespace

size_t attention_bwd_stats_bytes(int B, int H, int Sq) { return (size_t)B * H * ((Sq + TILE - 1) / TILE) * 128 * sizeof(float); }

// fused backward (head_dim 64): stats = attention_bwd_stats_bytes of scratch for the per-tile {L, delta} records (the dq kernel
// writes them, the dk,dv kernel reads them); a.lse from the training forward; O = a.o_bf16, or a.h_after - a.h_before
hipError_t launch_attention_bwd64(const AttnBwdArgs& a, float* stats, hipStream_t s) {
    if (a.dh != DH || a.B <= 0 || a.H <= 0 || a.Sq <= 0 || a.Skv <= 0 || !stats || !a.lse) return hipErrorInvalidValue;
    if ((a.ldq | a.ldk | a.ldv | a.lddo) % 8 || (a.lddq | a.lddk | a.lddv) % 4) return hipErrorInvalidValue;
    if (a.o_bf16 ? a.ldo % 8 != 0 : (!a.h_after || !a.h_before || a.ldh % 4 != 0)) return hipErrorInvalidValue;
    BwdParams p;
    p.q = (const bf16*)a.q; p.ldq = a.ldq; p.k = (const bf16*)a.k; p.ldk = a.ldk; p.v = (const bf16*)a.v; p.ldv = a.ldv;
    p.dout = (const bf16*)a.dout; p.lddo = a.lddo;
    p.dq = (bf16*)a.dq; p.lddq = a.lddq; p.dk = (bf16*)a.dk; p.lddk = a.lddk; p.dv = (bf16*)a.dv; p.lddv = a.lddv;
    p.stats = stats; p.lse = a.lse; p.o = (const bf16*)a.o_bf16; p.ldo = a.ldo;
    p.h_after = a.h_after; p.h_before = a.h_before; p.ldh = a.ldh;
    p.B = a.B; p.H = a.H; p.Sq = a.Sq; p.Skv = a.Skv;
    p.scale = a.scale; p.scale_log2 = a.scale * 1.4426950408889634f;
    p.drop_thr = dropout_threshold(a.dropout_p);
    p.keep_scale = p.drop_thr ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
    p.seed_lo = (unsigned)(a.seed & 0xFFFFFFFFu); p.seed_hi = (unsigned)(a.seed >> 32); p.layer = a.layer;
    p.rope_cos = a.rope_cos; p.rope_sin = a.rope_sin;
    if ((a.rope_cos == nullptr) != (a.rope_sin == nullptr) || (a.rope_cos && a.Sq != a.Skv)) return hipErrorInvalidValue;
    // diagnostic: DITTO_BWD_LDS_PAD=32768 pads the launch's LDS so that ONE workgroup fits a CU (one wave per SIMD): a lone wave's
    // timeline is serial, so knock-out builds (tools/bwd_knockout.sh) then read as additive shares of a tile's cycles
    static const int lds_pad = [] { const char* e = getenv("DITTO_BWD_LDS_PAD"); return e ? atoi(e) : 0; }();
    const int LDS0 = NBUF * 2 * IMG + lds_pad, LDS1 = NBUF * (2 * IMG + STAT_BYTES) + lds_pad;
    static DevOnce lds_once;
    if (hipError_t e = set_max_lds_once(lds_once, {reinterpret_cast<const void*>(&attn64_bwd_kernel<0, false, false>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<0, true, false>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<0, false, true>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<0, true, true>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<1, false>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<1, true>)}, LDS1 + 32768)) return e;
    const bool drop = p.drop_thr != 0, rag = (a.Skv & (TILE - 1)) != 0;
    p.nblk = (a.Sq + BLK - 1) / BLK;
    const dim3 g0(p.nblk * a.H * a.B), blk(256);
    if (drop && rag) hipLaunchKernelGGL((attn64_bwd_kernel<0, true, true>), g0, blk, LDS0, s, p);
    else if (drop) hipLaunchKernelGGL((attn64_bwd_kernel<0, true, false>), g0, blk, LDS0, s, p);
    else if (rag) hipLaunchKernelGGL((attn64_bwd_kernel<0, false, true>), g0, blk, LDS0, s, p);
    else hipLaunchKernelGGL((attn64_bwd_kernel<0, false, false>), g0, blk, LDS0, s, p);
    p.nblk = (a.Skv + BLK - 1) / BLK;
    if (drop) hipLaunchKernelGGL((attn64_bwd_kernel<1, true>), dim3(p.nblk * a.H * a.B), blk, LDS1, s, p);
    else hipLaunchKernelGGL((attn64_bwd_kernel<1, false>), dim3(p.nblk * a.H * a.B), blk, LDS1, s, p);
    return hipGetLastError();
}

}  // namespace ditto
