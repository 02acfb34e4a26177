// fr_common.h — what the hand-scheduled full-row kernels (gemm_frd.hip, gemm_fr64.hip, gemm_lnq.hip) have in common (gfx950).
//
// All three are one wave tile: 4 (lnq: or 8) waves side by side in N, wave wn owning ALL rows of the tile x its own columns as
// 32 x 32 blocks of v_mfma_f32_32x32x16_bf16 with the WEIGHTS as the instruction's A operand, so the accumulator is C^T: lane
// (r32 = lane & 31, hh = lane >> 5) holds, for row 32 mb + r32, the four columns 8 g + 4 hh .. + 3 of column block nb in
// elements 4 g .. 4 g + 3.  The accumulators are pinned in their register file by asm statements, because hipcc cannot be
// trusted with 192 .. 384 of them as values (it spills, or copies whole blocks between the files).
//
// Here: the MFMA statements, the pins, the W fragment load and its counted wait, LDS-DMA, the tile map, bias-row staging, and the
// pieces of gemm_frd's and gemm_fr64's accumulator init, residual window, LayerNorm row chain and store staging that are the
// same statement in both.  Everything is forced inline; each kernel file keeps its LDS layout, operand streaming, stage
// schedule, wait counts, diagnostic switches and launcher, and the loops that walk (nb, mb) around these pieces.
// tools/asm_identity.py checks that a change here leaves every kernel's machine code alone.  Forms that did NOT (r14): whole
// init / window / row-chain / store functions over a struct of both accumulator arrays (not narrowed further); gamma | beta
// through fr_stage_row; the store read-back loop taking the store as a lambda; fr_stage_bf16 for gemm_frd's bf16 h image.
#pragma once
#include <type_traits>   // fr_acc_init

#include "gemm_common.h"

namespace ditto {

// The accumulator's home file.  An asm operand constraint cannot depend on a template parameter, hence the overloads.
struct InAgpr {};
struct InVgpr {};

// c += w a, in place in c's home file.  W: a fragment as loaded (f32x4 from global memory, bf16x8 from the LDS).
template <typename W>
DITTO_DEV void fr_mfma(InAgpr, f32x16& c, const W& w, const bf16x8& a) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(w), "v"(a));
}
template <typename W>
DITTO_DEV void fr_mfma(InVgpr, f32x16& c, const W& w, const bf16x8& a) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(w), "v"(a));
}
// The LAST MFMA of an accumulator chain carries its own wait states: an 8-pass MFMA's result may be read by anything but
// the next MFMA of its chain only 11 cycles after issue, hipcc pads nothing behind an asm producer, and it DID place the
// spill of a just-written block between two MFMA statements (ahead of a separate s_nop statement: wrong lanes in u).
template <typename W>
DITTO_DEV void fr_mfma_last(InAgpr, f32x16& c, const W& w, const bf16x8& a) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\ts_nop 15" : "+a"(c) : "v"(w), "v"(a));
}
template <typename W>
DITTO_DEV void fr_mfma_last(InVgpr, f32x16& c, const W& w, const bf16x8& a) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\ts_nop 15" : "+v"(c) : "v"(w), "v"(a));
}

// Pin a value in its file: the statement "writes" x, so x must BE there at this point, and whatever reads x afterwards reads
// a new value that cannot be scheduled above it.  Re-pin an accumulator block right before it is copied out as a value
// (LayerNorm row chain, store epilogue): un-pinned, hipcc read four AGPR blocks into VGPRs at once right behind the barrier.
template <typename T>
DITTO_DEV void fr_pin(InAgpr, T& x) { asm volatile("" : "+a"(x)); }
template <typename T>
DITTO_DEV void fr_pin(InVgpr, T& x) { asm volatile("" : "+v"(x)); }

// W fragment straight from L2 into registers: 16 bytes per lane at base (scalar) + voff + IMM, not tracked by the compiler.
// (asm with operands lives in free functions: inside a generic lambda clang rejects asm operands that name captured locals)
template <int IMM>
DITTO_DEV void fr_wload(f32x4& dst, unsigned voff, const char* base) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(IMM) : "memory");
}
template <int VM>
DITTO_DEV void fr_wait(f32x4& frag) {   // counted wait that ties the fragment's registers: no use moves above it
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(frag) : "n"(VM) : "memory");
}

// LDS-DMA of one 1-KiB piece (64 lanes x 16 B from base + voff to LDS address dst + lane * 16).  Unlike glds16 it leaves M0
// clobbered: for the kernels that issue nothing else through M0.
DITTO_DEV void fr_dma(unsigned voff, const char* base, unsigned dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(dst) : "memory");
}

// XCD-contiguous tiles: workgroups go to the XCDs round-robin (blocks b and b + 8 share an XCD and its L2), so the workgroups
// of one XCD take neighbouring tiles — neighbouring rows and neighbouring K-loop phases.
DITTO_DEV int fr_xcd_tile() {
    const int ntile = gridDim.x;
    return (ntile & 7) == 0 ? (int)(blockIdx.x & 7) * (ntile >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
}

// The fp32 bias row of NP x 256 columns -> LDS at byte `off`, by ONE wave: NP LDS-DMA pieces of 1 KiB (the caller's vmcnt
// wait + barrier make them visible) ...
template <int NP>
DITTO_DEV void fr_stage_row(const float* src, unsigned lds_base, int off, int lane) {
#pragma unroll
    for (int i = 0; i < NP; ++i) glds16(src + i * 256 + lane * 4, lds_base + (unsigned)(off + i * 1024));
}
// ... or zeros there, where the launch has no bias
template <int NP>
DITTO_DEV void fr_zero_row(char* smem, int off, int lane) {
#pragma unroll
    for (int i = 0; i < NP; ++i) *reinterpret_cast<f32x4*>(smem + off + i * 1024 + lane * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// One 32 x 32 accumulator block's STARTING value: bias + residual, so that the epilogue only READS the accumulators.  t: the
// lane's residual values, four columns per g (fp32 x 4, or u32x2 = bf16 x 4 packed); b: the LDS bias row at the block's
// first column of this lane.  The caller assigns the value to the block's home file and pins it there.
template <typename R>
DITTO_DEV f32x16 fr_acc_init(const R (&t)[4], const float* b) {
    f32x16 v;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(b + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float r;
            if constexpr (std::is_same<R, u32x2>::value) r = __builtin_bit_cast(float, (e & 1) ? (t[g][e >> 1] & 0xFFFF0000u) : (t[g][e >> 1] << 16));
            else r = t[g][e];
            v[4 * g + e] = r + b4[e];
        }
    }
    return v;
}

// The fp32 residual of column block NB in the accumulator layout: four untracked 16-byte loads from the lane's row at the wave's
// column origin + 4 hh, and the counted wait that ties their registers (YOUNGER loads may stay in flight).
template <int NB, typename R>
DITTO_DEV void fr_res_load(R (&t)[4], const void* ptr) {
    asm volatile("global_load_dwordx4 %0, %4, off offset:%5\n\t"
                 "global_load_dwordx4 %1, %4, off offset:%6\n\t"
                 "global_load_dwordx4 %2, %4, off offset:%7\n\t"
                 "global_load_dwordx4 %3, %4, off offset:%8"
                 : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
                 : "v"(ptr), "n"(NB * 128), "n"(NB * 128 + 32), "n"(NB * 128 + 64), "n"(NB * 128 + 96)
                 : "memory");
}
template <int YOUNGER, typename R>
DITTO_DEV void fr_res_wait(R (&t)[4]) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]) : "n"(YOUNGER) : "memory");
}

// LayerNorm statistics, the lane's chain through a block's 16 elements: PASS 0 c += v, PASS 1 c += (v - rsum / N)^2 with both
// fused forms written out (left to the compiler, contraction follows basic-block structure, which differs between the kernels).
template <int PASS, int N>
DITTO_DEV void fr_row_acc(float& c, const f32x16& v, float rsum) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if constexpr (PASS == 0) c += v[e];
        else { const float dl = fmaf(rsum, -(1.0f / N), v[e]); c = fmaf(dl, dl, c); }
    }
}

// Store staging.  In the accumulator layout a store would touch 32 rows for 16 bytes each, so every output row leaves through a
// wave-private LDS image [rows][128 B] (16-byte chunk c of row r at c ^ (r & 7)) and is read back row-contiguous: whole lines.
// fp32 image (one column block per line): the lane's columns 8 g + 4 hh .. + 3 of `row`
DITTO_DEV void fr_stage_f32(char* st, int row, int g, int hh, f32x4 v) {
    *reinterpret_cast<f32x4*>(st + row * 128 + (((2 * g + hh) ^ (row & 7)) << 4)) = v;
}
// bf16 image (two column blocks per line): the same columns of block nb as packed bf16
DITTO_DEV void fr_stage_bf16(char* st, int row, int nb, int g, int hh, f32x4 v) {
    u32x2 s;
    s[0] = pack_bf16x2(v[0], v[1]); s[1] = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(st + row * 128 + ((((nb & 1) * 4 + g) ^ (row & 7)) << 4) + hh * 8) = s;
}

DITTO_DEV int fr_store_m(const GemmParams& p) {   // rows below this are stored (-DDITTO_DIAG_FR_NOSTORE: none, timing only)
#ifdef DITTO_DIAG_FR_NOSTORE
    return p.M - (1 << 30);
#endif
    return p.M;
}

}  // namespace ditto
