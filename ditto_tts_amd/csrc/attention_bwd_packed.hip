// attention_bwd_packed.hip — the packed instantiations of the fused attention backward (attn64bwd.h; algorithm: attention_bwd.hip):
// utterances concatenated along the rows, utterance b owning rows [cu_q[b], cu_q[b+1]) of q / dO / O / dq and [cu_kv[b], cu_kv[b+1])
// of k / v / dk / dv — the layout the packed training step keeps its tape in (reference src/components/DiT.py:131-148 under autograd,
// one utterance at a time: no key of a neighbour, no padding key, is ever part of a softmax).
//   grid      blocks of 128 rows of the LONGEST utterance x H x B; a workgroup whose block starts past its utterance's end leaves at once
//   keys      the dq kernel masks keys past the utterance's own count (always compiled in: which utterance is ragged is not a property of
//             the launch); the dk,dv kernel's tile rows are queries, and rows past the utterance's count carry L = 1e30 (P = 0)
//   records   {L, delta} per (head, 64-query tile): utterance b's tiles from record (cu_q[b] >> 6) + b on — floor(cu / 64) + b grows by at
//             least ceil(N_b / 64) per utterance, so no prefix sum is needed and S / 64 + B + 1 records per head hold them all
//   stores    dq / dk / dv of the utterance's own rows only: a 128-row block that runs past its end overlaps the NEXT utterance's rows
//   RoPE      the inverse rotation in the dq / dk epilogues at the row's position inside its utterance; dropout mask: the hash on
//             stream b H + h at the utterance-local (query, key) indices
// Its own translation unit (build.py EXTRA, as attention_bwd.hip): the dense kernels keep their ISA.
#include <type_traits>

#include "gemm_common.h"

#define DITTO_BWD_PACKED 1

namespace ditto {

namespace {
namespace packed {
#include "attn64bwd.h"
}  // namespace packed
}  // namespace

size_t attention_bwd_stats_bytes_packed(int B, int H, int q_rows) {
    return (size_t)H * ((size_t)q_rows / packed::TILE + B + 1) * 128 * sizeof(float);
}

hipError_t launch_attention_bwd64_packed(const AttnBwdArgs& a, float* stats, hipStream_t s) {
    using namespace packed;
    if (a.dh != DH || a.B <= 0 || a.H <= 0 || a.Sq <= 0 || a.Skv <= 0 || !stats || !a.lse || !a.o_bf16) return hipErrorInvalidValue;
    if (!a.cu_q || !a.cu_kv || a.q_rows <= 0 || a.kv_rows <= 0 || a.Sq > a.q_rows || a.Skv > a.kv_rows) return hipErrorInvalidValue;
    if ((a.ldq | a.ldk | a.ldv | a.lddo | a.ldo) % 8 || (a.lddq | a.lddk | a.lddv) % 4) return hipErrorInvalidValue;
    if ((a.rope_cos == nullptr) != (a.rope_sin == nullptr)) return hipErrorInvalidValue;
    BwdParams p;
    p.q = (const bf16*)a.q; p.ldq = a.ldq; p.k = (const bf16*)a.k; p.ldk = a.ldk; p.v = (const bf16*)a.v; p.ldv = a.ldv;
    p.dout = (const bf16*)a.dout; p.lddo = a.lddo;
    p.dq = (bf16*)a.dq; p.lddq = a.lddq; p.dk = (bf16*)a.dk; p.lddk = a.lddk; p.dv = (bf16*)a.dv; p.lddv = a.lddv;
    p.stats = stats; p.lse = a.lse; p.o = (const bf16*)a.o_bf16; p.ldo = a.ldo;
    p.h_after = nullptr; p.h_before = nullptr; p.ldh = 0;
    p.B = a.B; p.H = a.H; p.Sq = a.Sq; p.Skv = a.Skv;
    p.scale = a.scale; p.scale_log2 = a.scale * 1.4426950408889634f;
    p.drop_thr = dropout_threshold(a.dropout_p);
    p.keep_scale = p.drop_thr ? 1.0f / (1.0f - a.dropout_p) : 1.0f;
    p.seed_lo = (unsigned)(a.seed & 0xFFFFFFFFu); p.seed_hi = (unsigned)(a.seed >> 32); p.layer = a.layer;
    p.rope_cos = a.rope_cos; p.rope_sin = a.rope_sin;
    p.cu_q = a.cu_q; p.cu_kv = a.cu_kv; p.q_rows = a.q_rows; p.kv_rows = a.kv_rows;
    p.nrec = a.q_rows / TILE + a.B + 1;
    const int LDS0 = NBUF * 2 * IMG, LDS1 = NBUF * (2 * IMG + STAT_BYTES);
    static DevOnce lds_once;
    if (hipError_t e = set_max_lds_once(lds_once, {reinterpret_cast<const void*>(&attn64_bwd_kernel<0, false, true>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<0, true, true>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<1, false>),
                                                   reinterpret_cast<const void*>(&attn64_bwd_kernel<1, true>)}, LDS1)) return e;
    const bool drop = p.drop_thr != 0;
    const dim3 blk(256);
    p.nblk = (a.Sq + BLK - 1) / BLK;
    if (drop) hipLaunchKernelGGL((attn64_bwd_kernel<0, true, true>), dim3(p.nblk * a.H * a.B), blk, LDS0, s, p);
    else hipLaunchKernelGGL((attn64_bwd_kernel<0, false, true>), dim3(p.nblk * a.H * a.B), blk, LDS0, s, p);
    p.nblk = (a.Skv + BLK - 1) / BLK;
    if (drop) hipLaunchKernelGGL((attn64_bwd_kernel<1, true>), dim3(p.nblk * a.H * a.B), blk, LDS1, s, p);
    else hipLaunchKernelGGL((attn64_bwd_kernel<1, false>), dim3(p.nblk * a.H * a.B), blk, LDS1, s, p);
    return hipGetLastError();
}

}  // namespace ditto
