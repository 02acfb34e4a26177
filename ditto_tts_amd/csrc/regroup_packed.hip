// regroup_packed.hip — change the membership of a packed batch on the device (gfx950): one launch, driven by a segment table,
// builds the next batch's state, conditioning image and offsets from the current buffers plus the newcomers', and copies out the
// rows of the utterances that leave (continuous batching, ditto_tts_amd/serving.py).  Pure 16-byte copies — the result is bit-exact
// — and, for a newcomer that starts from its seed, ditto_noise_normal's numbers at the x_T tag.
#include "common.h"
#include "ditto_hip.h"
#include "kernels.h"
#include "philox.h"

namespace ditto {

// Segment blockIdx.y of `table` (ditto_regroup_seg, include/ditto_hip.h): `n` 16-byte units from source buffer `source` at unit
// `src_off` (kind 0), or normal4(seeds[aux], 0xFFFFFFFF, i) for unit i of the segment (kind 1: the segment is one utterance's whole
// x_T, so i is the utterance-local quad index), to destination buffer `dest` at unit `dst_off` and, when dup_off != 0, also at
// dst_off + dup_off (the unconditional half under CFG).  Every index, offset and length is clamped into the buffers the call was
// given: a bad table gives wrong rows, never an access outside them.  The buffer of an index is picked by compare-and-select over
// the constant indices (no dynamic indexing of the argument struct, hence no scratch).
__global__ __launch_bounds__(256) void regroup_packed_kernel(const ditto_regroup_seg* __restrict__ table, RegroupBufs bufs,
                                                             const int64_t* __restrict__ seeds, int n_seeds) {
    const ditto_regroup_seg sg = table[blockIdx.y];
    const f32x4* sp = nullptr;
    f32x4* dp = nullptr;
    unsigned sn = 0, dn = 0;
#pragma unroll
    for (int k = 0; k < DITTO_REGROUP_BUFS; ++k) {
        if (sg.source == k) { sp = reinterpret_cast<const f32x4*>(bufs.src[k]); sn = bufs.src_n[k]; }
        if (sg.dest == k) { dp = reinterpret_cast<f32x4*>(bufs.dst[k]); dn = bufs.dst_n[k]; }
    }
    if (!dp) return;
    const unsigned long long d1 = (unsigned long long)sg.dst_off + sg.dup_off;     // the last unit written is d1 + n - 1
    if (d1 >= dn) return;
    unsigned n = sg.n < dn - (unsigned)d1 ? sg.n : dn - (unsigned)d1;
    f32x4* d0p = dp + sg.dst_off;
    f32x4* d1p = dp + d1;
    const bool dup = sg.dup_off != 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (sg.kind == 1) {
        if (!seeds || n_seeds <= 0) return;
        const int si = sg.aux < 0 ? 0 : (sg.aux > n_seeds - 1 ? n_seeds - 1 : sg.aux);
        const unsigned long long seed = (unsigned long long)seeds[si];
        for (; i < n; i += stride) {
            const f32x4 z = normal4(seed, 0xFFFFFFFFu, i);
            d0p[i] = z;
            if (dup) d1p[i] = z;
        }
        return;
    }
    if (!sp || sg.src_off >= sn) return;
    n = n < sn - sg.src_off ? n : sn - sg.src_off;
    const f32x4* s0p = sp + sg.src_off;
    for (; i + 3 * stride < n; i += 4 * stride) {      // four loads in flight per lane
        const f32x4 v0 = s0p[i], v1 = s0p[i + stride], v2 = s0p[i + 2 * stride], v3 = s0p[i + 3 * stride];
        d0p[i] = v0; d0p[i + stride] = v1; d0p[i + 2 * stride] = v2; d0p[i + 3 * stride] = v3;
        if (dup) { d1p[i] = v0; d1p[i + stride] = v1; d1p[i + 2 * stride] = v2; d1p[i + 3 * stride] = v3; }
    }
    for (; i < n; i += stride) {
        const f32x4 v = s0p[i];
        d0p[i] = v;
        if (dup) d1p[i] = v;
    }
}

hipError_t launch_regroup_packed(const ditto_regroup_seg* table, int n_seg, const RegroupBufs& bufs, const int64_t* seeds, int n_seeds,
                                 size_t max_units, hipStream_t s) {
    if (!table || n_seg <= 0 || n_seg > 65535) return hipErrorInvalidValue;
    size_t gx = (max_units + 1023) / 1024;
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    hipLaunchKernelGGL(regroup_packed_kernel, dim3((unsigned)gx, n_seg), dim3(256), 0, s, table, bufs, seeds, n_seeds);
    return hipGetLastError();
}

}  // namespace ditto
