// attention_train_packed.hip — the training forward's fused attention (attention_train.hip: attn64v2 <TRAIN[, DROP]>) over a PACKED batch:
// utterances concatenated along the rows, utterance b owning rows [cu_q[b], cu_q[b+1]) of q / out / resid and [cu_kv[b], cu_kv[b+1]) of
// k / v (reference src/components/DiT.py:131-148, one utterance at a time).  DITTO_ATTN_V2_PACKED makes attn64v2.h take an utterance's
// first rows and lengths from the offsets: the key loop runs over its own key count with the last tile masked, queries past its own count
// are neither loaded as valid nor stored, the log2-domain log-sum-exp goes to lse [H, q_rows] at the packed query row, and the dropout
// mask is the hash on stream b H + h at the utterance-local (query, key) indices.  Grid: blocks of 128 queries of the longest utterance.
// Its own translation unit, compiled like attention_train.hip (build.py EXTRA), so that the dense kernels keep their ISA.
#include <type_traits>

#include "attn_common.h"

#define DITTO_ATTN_V2_PACKED 1

namespace ditto {

namespace {
namespace packed {
#include "attn64v2.h"
}  // namespace packed
}  // namespace

// p.nqb is set here.  Both forms of the training step: plain -> bf16 O (cross-attention, with dropout) and the residual epilogue (self-
// attention; fp32 stream, or bf16 stream with O written beside it when p.out is set)
hipError_t launch_attention_train64_packed(const AttnParams& p_in, bool resid, hipStream_t s) {
    if (!p_in.cu_q || !p_in.cu_kv || p_in.q_rows <= 0 || p_in.kv_rows <= 0 || p_in.Sq > p_in.q_rows || p_in.Skv > p_in.kv_rows)
        return hipErrorInvalidValue;
    using namespace packed;
    AttnParams p = p_in;
    p.nqb = (p.Sq + QBLK - 1) / QBLK;
    const dim3 grid(p.nqb * p.H * p.B), block(256);
    if (p.drop_thr) {
        if (resid) hipLaunchKernelGGL((attn64v2_kernel<true, 3, 2, true, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((attn64v2_kernel<false, 3, 2, true, true>), grid, block, 0, s, p);
    } else {
        if (resid) hipLaunchKernelGGL((attn64v2_kernel<true, 3, 2, true, false>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((attn64v2_kernel<false, 3, 2, true, false>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace ditto
