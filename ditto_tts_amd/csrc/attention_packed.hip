// attention_packed.hip — the packed instantiations of attn64q / attn64p (attn64q.h, attn64p.h): utterances concatenated along the
// rows, utterance b owning rows [cu_q[b], cu_q[b+1]) of q / out / resid and [cu_kv[b], cu_kv[b+1]) of k / v (flash-attention's varlen
// layout).  DITTO_ATTN_PACKED makes the headers take an utterance's first rows from the offsets instead of b * Sq / b * Skv; all else
// is the VARLEN masking of attention_varlen.hip (Sq / Skv: the longest lengths, the grid), so an utterance gets the same arithmetic
// as in the padded varlen kernel.  Rows outside an utterance's own range — other utterances' included — are never read or written.
// Its own translation unit, compiled like attention_varlen.hip (build.py EXTRA), so that the dense and padded kernels keep their ISA.
#include <type_traits>

#include "attn_common.h"

#define DITTO_ATTN_PACKED 1

namespace ditto {

namespace {
namespace packed {
#include "attn64v2.h"   // the tile constants
#include "attn64p.h"
#include "attn64q.h"
}  // namespace packed
}  // namespace

// p.nqb is set here: blocks of 256 queries of the longest utterance.  The launch choices of launch_attn64p_varlen.
hipError_t launch_attn64p_packed(const AttnParams& p_in, bool resid, hipStream_t s, bool exact_only) {
    if (!p_in.cu_q || !p_in.cu_kv || p_in.q_rows <= 0 || p_in.kv_rows <= 0) return hipErrorInvalidValue;
    using namespace packed;
    AttnParams p = p_in;
    p.nqb = (p.Sq + 255) / 256;
    const dim3 grid(p.nqb * p.H * p.B), block(256);
    if (exact_only) {
        if (resid) hipLaunchKernelGGL((attn64p_kernel<true, 4, 0, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((attn64p_kernel<false, 4, 0, true>), grid, block, 0, s, p);
    } else if (resid) {
        hipLaunchKernelGGL((attn64q_kernel<true, 0, Q_QD, true, 0, true, true>), grid, block, 0, s, p);
    } else {
        hipLaunchKernelGGL((attn64q_kernel<false, 0, Q_QD, true, 0, true, true>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace ditto
