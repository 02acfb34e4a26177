// attention_varlen.hip — the VARLEN instantiations of attn64q / attn64p (attn64q.h, attn64p.h): variable-length batches, every
// utterance bounded by its own query / key lengths (p.q_len / p.kv_len) in the padded layout.  Their own translation unit, compiled
// like attention_p.hip (build.py EXTRA: -fno-honor-nans -fno-slp-vectorize): co-compiled kernel templates perturb one another's
// register allocation (guide rule 19), and the dense kernels of attention_p.hip keep their ISA.
#include <type_traits>

#include "attn_common.h"

namespace ditto {

namespace {
#include "attn64v2.h"   // the tile constants
#include "attn64p.h"
#include "attn64q.h"
}  // namespace

// p.nqb is set here: blocks of 256 queries.  Always this family, whatever the grid: attn64q, with attn64p's body for the workgroups
// whose utterance has one key tile, or attn64p alone (exact_only: attn_flags 1048576).  No fragment hold and no ring of 3: the
// partial last tile is data, not shape, so every varlen launch takes the RAGGED instantiation.
hipError_t launch_attn64p_varlen(const AttnParams& p_in, bool resid, hipStream_t s, bool exact_only) {
    if (!p_in.q_len && !p_in.kv_len) return hipErrorInvalidValue;
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
