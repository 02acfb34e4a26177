// philox.h — the library's counter-based N(0,1) generator, shared by the kernels that draw per-utterance noise
// (rowwise.hip: noise_normal / p_sample_update_seeded; guided.hip: the fused guided update).  One definition, so every
// kernel that draws element i of utterance b at a step gets the same bits.
#pragma once
#include "common.h"

namespace ditto {

// ------------------------------------------------------------------------------------------------
// Per-utterance counter-based N(0,1): Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; the Random123 constants) keyed by the utterance's 64-bit seed, counter = (element quad, step, stream), then
// Box-Muller on the four 32-bit words.  Element i of utterance b at step s depends on (seed[b], s, i) ONLY — not on
// the batch the utterance sits in, its position in it, or the GPU: what makes batch-sharded sampling reproduce the
// unsharded result bit for bit.  The reference draws from torch's global generator
// (src/model/SpeechGenerator.py:141,154), whose stream cannot be sharded; that path stays the default.
// ------------------------------------------------------------------------------------------------
DITTO_DEV void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
// four N(0,1) of (seed, step, quad index): u = ((word >> 8) + 0.5) 2^-24 in (0,1) (the top 24 bits of a Philox word);
// r = sqrt(-2 ln u1); angle = 2 pi u2
DITTO_DEV f32x4 normal4(unsigned long long seed, unsigned step, unsigned long long quad) {
    unsigned w[4];
    philox4x32_10((unsigned)quad, (unsigned)(quad >> 32), step, 0x44695454u /* "DiTT" */, (unsigned)seed,
                  (unsigned)(seed >> 32), w);
    f32x4 z;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(w[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);        // 24 bits: exact in fp32, never 0 or 1
        const float u2 = ((float)(w[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float r = __fsqrt_rn(-1.3862943611198906f * __builtin_amdgcn_logf(u1));  // -2 ln u = -2 ln2 log2 u
        z[2 * h] = r * __builtin_amdgcn_cosf(u2);                                        // v_cos / v_sin take revolutions
        z[2 * h + 1] = r * __builtin_amdgcn_sinf(u2);
    }
    return z;
}

}  // namespace ditto
