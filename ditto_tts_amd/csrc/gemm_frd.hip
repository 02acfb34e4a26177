// gemm_frd.hip — the full-row N = 768 GEMM with fused residual + LayerNorm (gemm_fr.hip's contract) with the WEIGHTS
// FETCHED STRAIGHT FROM L2 INTO REGISTERS: no W ring in the LDS, no LDS-DMA and no ds_read for the large operand (gfx950).
//
//     h[M, 768] (fp32, in place) = residual + A[M, K] * W[768, K]^T + bias            (reference DiT.py:148, :155)
//     u[M, 768] (bf16)           = LayerNorm(h) * gamma + beta   (eps 1e-5)           (reference DiT.py:152, :105)
//
// (gemm_fr128 = the 128-row kernel of rounds 2-5 with the weights through an LDS ring, deleted in round 6; it lived in gemm_fr.hip, now the
// dispatcher.)  Why: gemm_fr128's main loop ran at 0.55 us per K = 16 stage where its 24 MFMAs need 0.40: the 24 KiB of W per stage go
// L2 -> LDS by LDS-DMA (the path sustains ~52 GB/s per CU next to MFMAs and fragment reads) and come back out through 12
// ds_read_b128 per wave and stage behind a barrier per stage.  The weights are packed stage-major, Wp[K/16][768][16], so the
// 1 KiB of a (stage, 32-column block) piece is contiguous and lane (r32, hh) of a v_mfma_f32_32x32x16_bf16 operand wants
// exactly the 16 bytes at r32 * 32 + hh * 16 of it: ONE global_load_dwordx4 per fragment whose wave covers eight whole cache
// lines.  tools/probe_wdirect.hip measured that stream at 105 GB/s per CU alone and at 0.44-0.50 us per stage with the 24 MFMAs,
// two stages of look-ahead being the best depth.  That needs W to be wave-private, hence another wave tile:
//
//   tile      128 rows x 768 columns, one workgroup per CU, 4 waves side by side in N: wave wn owns ALL 128 rows x columns
//             [192 wn, +192) = 4 x 6 blocks of 32 x 32 = 384 accumulators (column blocks 0..3 in AGPRs = 256, 4..5 in VGPRs).
//   W         six fragments per stage and wave, a register ring of two stages (48 VGPRs); fragment nb of stage s+2 is
//             loaded into the registers of fragment nb of stage s right behind the four MFMAs that consumed it.  Every
//             fragment is waited for separately with a counted vmcnt (11 younger loads + the A pieces issued since: a
//             compile-time constant per (slab position, nb)), so each load has its full two stages to land.
//   A         shared by the four waves, through the LDS as in gemm_fr128: slabs of 64 k (128 rows x 128 B = 16 pieces of
//             1 KiB, 4 per wave, chunk c of row r at c ^ ((r >> 1) & 7)), double-buffered, ONE barrier per slab; 4
//             ds_read_b128 per wave and stage (gemm_fr128: 14).
//   K order   as gemm_fr128 (rotation per 128-row tile included): h is bit-identical to gemm_fr128's.  The LayerNorm
//             statistics are summed per quarter row ((q0 + q1) + (q2 + q3)), so u may differ from gemm_fr128's in the last
//             bf16 bit of a few elements.
//   residual  bf16 stream (the model path): the tile's 192 KiB reach the accumulators THROUGH THE LDS — every wave fetches its own
//             384 bytes of each row by LDS-DMA in whole 128-byte lines (48 pieces of 1 KiB per wave, two 32-row units in flight)
//             and reads them back in the accumulator layout (96 ds_read_b64 per lane).  In-model the launch went 66.5 -> 62.0 us
//             (K = 768) and 137.6 -> 132.7 us (K = 3072); with no residual read at all it would be 55.8 / 121.4
//             (profiles/r13_frd_res_ceiling.txt).  The fp32 stream keeps its loads in the accumulator layout.
//   LDS       A 2 x 16 KiB + bias row 3 KiB in the loop, the residual staging (4 waves x 2 x 12 KiB) behind them in the prologue;
//             the epilogue stages every output row through a wave-private 32 KiB (whole-line stores) + gamma | beta + row
//             statistics: 138 KiB.
#include <type_traits>

#include "fr_common.h"

namespace ditto {

namespace {

constexpr int DM = 128, DN = 768, DK = 16;
constexpr int D_W_BYTES = DN * DK * 2;              // 24 KiB: one K = 16 stage of W in memory
constexpr int D_ASLAB = DM * 64 * 2;                // 16 KiB: 128 rows x 64 k
constexpr int D_BIAS = 2 * D_ASLAB;                 // bias row (3 KiB) behind the two A slabs
constexpr int D_STAGE = 4 * 32768;                  // epilogue: 4 x 32 KiB of store staging (overlays A and bias) ...
constexpr int D_GB = D_STAGE;                       // ... gamma | beta rows (6 KiB) ...
constexpr int D_RED = D_GB + 2 * DN * 4;            // ... row sums [4 quarters][128 rows] fp32 (2 KiB)
constexpr int D_LDS = D_RED + 4 * DM * 4;           // 138 KiB
constexpr int DNA = 4;                              // column blocks (of 6) whose accumulators live in AGPRs
// prologue, bf16 stream: the residual tile comes through the LDS in whole 128-byte lines.  Per wave two buffers of one UNIT =
// 32 rows (one mb block) x this wave's 384 bytes of the row, as three [32 rows][128 B] images (16-byte chunk c of row r at
// c ^ ((r >> 1) & 7), the A slabs' swizzle, applied on the DMA's source address); idle in the main loop, under the epilogue's staging
constexpr int D_RSTG = D_BIAS + DN * 4;
constexpr int D_RUNIT = 32 * 384;                   // 12 KiB = 12 LDS-DMA pieces of 8 rows x 128 B
static_assert(D_RSTG % 128 == 0 && D_RUNIT % 128 == 0 && D_RSTG + 4 * 2 * D_RUNIT <= D_LDS, "residual staging fits under the epilogue's");

template <int IMM>
DITTO_DEV void frd_wload(f32x4& dst, unsigned voff, const char* base) {
#ifndef DITTO_DIAG_FRD_NOW      // tools/build_diag.sh: the main loop without its W stream (timing only, wrong results)
    fr_wload<IMM>(dst, voff, base);
#else
    asm volatile("" : "+v"(dst) : "v"(voff), "s"(base));
#endif
}
DITTO_DEV void frd_dma(unsigned voff, const char* base, unsigned dst) {   // fr_dma with the A stream's A/B switches
#ifndef DITTO_DIAG_FR_NODMA
#ifndef DITTO_FRD_A_POLICY     // A/B builds: cache policy of the A slab stream (tools/build_diag.sh -DDITTO_FRD_A_POLICY='"nt"')
#define DITTO_FRD_A_POLICY ""
#endif
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 " DITTO_FRD_A_POLICY ::"v"(voff), "s"(base), "s"(dst) : "memory");
#endif
}

// Vector-memory operations a wave has issued AFTER the load of W fragment (s, nb) when MFMA (s, nb) is about to issue, i.e.
// what may stay in flight at that wait.  Issue order of a stage at slab position j: W0 W1 W2 W3 W4 [A] W5 [A]  (the two A
// pieces only at j < 2 and while a next slab exists), W = the fragments of stage s + 2 while that stage exists.
//   last: this is the last slab (no A issue; stages 2, 3 issue no W).
constexpr int frd_vm(int j, int nb, bool last) {
    int c = 5 - nb;                                                   // stage s-2: W(s, nb+1 .. 5)
    const int j2 = (j + 2) & 3, j1 = (j + 3) & 3;
    const bool a_prev2 = j >= 2 ? !last : true, a_prev1 = j >= 1 ? !last : true, a_this = !last;
    if (a_prev2 && j2 < 2) c += nb <= 4 ? 2 : 1;                     //           its A pieces behind W4 / W5
    const bool w_prev1 = !(last && j == 3), w_this = !(last && j >= 2);
    if (w_prev1) c += 6;                                              // stage s-1: W(s+1, 0 .. 5)
    if (a_prev1 && j1 < 2) c += 2;
    if (w_this) c += nb;                                              // stage s:   W(s+2, 0 .. nb-1)
    if (a_this && j < 2 && nb == 5) c += 1;                           //            the A piece behind W4
    return c;
}
static_assert(frd_vm(0, 0, false) == 11 && frd_vm(0, 5, false) == 12 && frd_vm(1, 0, false) == 13 && frd_vm(2, 0, false) == 15 &&
              frd_vm(2, 5, false) == 14 && frd_vm(3, 4, false) == 13 && frd_vm(3, 5, false) == 12, "steady-state wait counts");
static_assert(frd_vm(0, 3, true) == 11 && frd_vm(2, 0, true) == 11 && frd_vm(2, 5, true) == 6 && frd_vm(3, 0, true) == 5 &&
              frd_vm(3, 5, true) == 0, "last-slab wait counts");

// HB: the residual stream is bf16 in HBM (fp.hb): residual read and h written as bf16 (fp32 only in the accumulators and the
// LayerNorm, which still sees the UNROUNDED fp32 row); p.residual / p.out point to bf16, ldr / ldo in bf16 elements.
#ifdef DITTO_DIAG_FRD_STAMP   // tools/build_diag_one.sh ... gemm_frd.hip -DDITTO_DIAG_FRD_STAMP: s_memtime stamps around the kernel's phases
__device__ unsigned long long g_frd_stamps[1024 * 4 * 8];
DITTO_DEV unsigned long long frd_now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define FRD_STAMP(i) const unsigned long long frd_t##i = frd_now()
#else
#define FRD_STAMP(i)
#endif

// accumulator-init group gi of 24 -> its (nb, mb) block (see the kernel's prologue)
constexpr int frd_group_nb(int gi) { return gi >> 2; }
constexpr int frd_group_mb(int gi) { return gi & 3; }
#ifdef DITTO_DIAG_FRD_NORES   // stamps only: the accumulators start from the bias alone (valid numbers, WRONG results) — what do the residual loads cost?
constexpr bool FRD_NORES = true;
#else
constexpr bool FRD_NORES = false;
#endif

template <bool LN, bool RES, bool HB = false>
__global__ __launch_bounds__(256, 1) void gemm_frd_kernel(FrParams fp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    FRD_STAMP(0);
    const GemmParams& p = fp.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);       // = the wave's column quarter
    const int nkt = p.K / DK;                                        // a multiple of 4 (K % 64 == 0)
    const int nslab = nkt >> 2;
    // XCD-contiguous tiles and the K-loop rotation: the same for every N = 768 kernel (same sums in the same order)
    const int tile = fr_xcd_tile();
    const int m0 = tile * DM;
    const int s0 = fp.rot_period > 0 ? (((tile % fp.rot_period) & 7) * nslab) >> 3 : 0;
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)smem;

    // ---- A: LDS-DMA in slabs of 64 k, 4 pieces (8 rows x 128 B) per wave and slab ----
    const int arow = lane >> 3, apos = lane & 7;
    unsigned vak[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 8 * (wid * 4 + j) + arow;
        int ar = m0 + row;
        ar = ar < p.M ? ar : p.M - 1;
#ifdef DITTO_DIAG_FR_AHOT      // tools/build_diag.sh: every tile reads the A rows of tile 0 (L2-resident, statistically the same data): what does A's HBM / Infinity Cache latency cost?
        ar = row;
#endif
        vak[j] = (unsigned)(((size_t)ar * p.lda + (apos ^ ((row >> 1) & 7)) * 8) * 2) + (unsigned)(s0 * 128);
    }
    int a_left = nslab - s0;                                          // slabs until the rotated K loop wraps to k = 0
    unsigned a_buf = lds_base;                                        // LDS address of the buffer the next slab goes to
    auto issue_a_piece = [&](auto J) {
        constexpr int j = decltype(J)::value;
        frd_dma(vak[j], (const char*)p.A, a_buf + (unsigned)((wid * 4 + j) * 1024));
    };
    auto advance_a = [&]() {
        a_buf = a_buf == lds_base ? lds_base + D_ASLAB : lds_base;
        --a_left;
        const unsigned inc = a_left == 0 ? 128u - (unsigned)nslab * 128u : 128u;
#pragma unroll
        for (int j = 0; j < 4; ++j) vak[j] += inc;
    };

    // ---- W: straight into registers.  Fragment (stage, nb) of this wave = the 1 KiB at stage * 24 KiB + (6 wn + nb) KiB of the
    //      stage-major image; lane (r32, hh) takes its 16 bytes at r32 * 32 + hh * 16.  One per-lane offset for nb 0..3
    //      (immediate nb * 1024), one 4 KiB further for nb 4, 5; both advance 24 KiB per stage and wrap with the rotation. ----
    const int r32 = lane & 31, hh = lane >> 5;
    unsigned vw0 = (unsigned)(wid * 6 * 1024 + r32 * 32 + hh * 16) + (unsigned)s0 * 4u * D_W_BYTES;
    int w_left = nkt - 4 * s0;
    f32x4 wr[2][6];                                                   // the register ring: [stage & 1][nb]
    auto issue_w = [&](auto NB, f32x4& dst) {
        constexpr int nb = decltype(NB)::value;
        if constexpr (nb < 4) frd_wload<nb * 1024>(dst, vw0, (const char*)p.W);
        else frd_wload<(nb - 4) * 1024>(dst, vw0 + 4096u, (const char*)p.W);
    };
    auto wait_frag = [&](auto VM, f32x4& frag) { fr_wait<decltype(VM)::value>(frag); };
    auto advance_w = [&]() {
        --w_left;
        vw0 += w_left == 0 ? (unsigned)D_W_BYTES - (unsigned)nkt * D_W_BYTES : (unsigned)D_W_BYTES;
    };

    // bias row -> LDS (3 pieces of 1 KiB): the oldest loads of the kernel
    if (wid == 0) {
        if (p.bias) fr_stage_row<3>(p.bias, lds_base, D_BIAS, lane);
        else fr_zero_row<3>(smem, D_BIAS, lane);
    }
    // A slab 0 (in flight while the accumulators are initialised)
    issue_a_piece(IntC<0>{}); issue_a_piece(IntC<1>{}); issue_a_piece(IntC<2>{}); issue_a_piece(IntC<3>{});
    advance_a();

    // A fragment addressing: row (32 mb + r32) x 128 B; stage j of the slab = 16-B chunks 2 j + hh
    const int a_row = r32 * 128;                                      // + mb * 4096
    const int a_x = (hh ^ ((r32 >> 1) & 7)) << 4;                     // ^ (j << 5)

    // ---- accumulators START as bias + residual (the epilogue only READS them) ----
    const float* lbias = reinterpret_cast<const float*>(smem + D_BIAS);
    const float* lgamma = reinterpret_cast<const float*>(smem + D_GB);     // these two: valid in the epilogue only
    const float* lbeta = lgamma + DN;
    f32x16 acca[DNA][4], accv[6 - DNA][4];
    using res_t = typename std::conditional<HB, u32x2, f32x4>::type;   // four columns of one row: bf16 x 4 or fp32 x 4
    // block (nb, mb) = bias + the residual values t (four columns per g), into its home file
    auto init_block = [&](auto NB, auto MB, const res_t (&t)[4]) {
        constexpr int nb = decltype(NB)::value, mb = decltype(MB)::value;
        const f32x16 v = fr_acc_init(t, lbias + wid * 192 + nb * 32 + 4 * hh);
        if constexpr (nb < DNA) { acca[nb < DNA ? nb : 0][mb] = v; fr_pin(InAgpr{}, acca[nb < DNA ? nb : 0][mb]); }
        else { accv[nb < DNA ? 0 : nb - DNA][mb] = v; fr_pin(InVgpr{}, accv[nb < DNA ? 0 : nb - DNA][mb]); }
        __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (RES && HB && !FRD_NORES) {
        // The bf16 stream (the model path).  In the accumulator layout a wave instruction would touch 32 rows for 16 bytes each:
        // 12 288 sixteen-byte requests per tile (measured at 2.9 TB/s, 14-16 % over-fetch).  Instead every wave stages ITS 384
        // bytes of each row through the LDS by LDS-DMA — three whole 128-byte lines per row, eight lines per instruction — one
        // unit of 32 rows at a time into two buffers, and reads it back in the accumulator layout with ds_read_b64 (chunk
        // (nb & 1) * 4 + g of image nb >> 1; the swizzle leaves the 32 rows of a read on 16 different chunk slots).  Wave-private:
        // no barrier, the wave's own counted vmcnt orders its reads behind its DMA.  Unit mb + 2 is issued into the buffer of
        // unit mb once that one has been read, so two units (24 KiB per wave) are in flight while one is converted.
        // Everything is retired by the vmcnt(0) below: the main loop's counts (frd_vm) see A and W only, as before.
        const unsigned rs_wave = lds_base + (unsigned)(D_RSTG + wid * 2 * D_RUNIT);
        const char* rs_rd = smem + D_RSTG + wid * 2 * D_RUNIT;
        const unsigned rd_off = (unsigned)(r32 * 128 + (((r32 >> 1) & 7) << 4) + hh * 8);     // ^ (chunk << 4)
        const unsigned rs_col = (unsigned)(wid * 384);
        auto issue_unit = [&](auto MB) {
            constexpr int mb = decltype(MB)::value;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {                                  // piece = 8 rows x 128 B: lane -> (row, position)
                const int row = rb * 8 + (lane >> 3);
                int gr = m0 + mb * 32 + row;
                gr = gr < p.M ? gr : p.M - 1;
                const unsigned voff = (unsigned)gr * (unsigned)p.ldr * 2u + rs_col + (unsigned)(((lane & 7) ^ ((row >> 1) & 7)) << 4);
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    fr_dma(voff + (unsigned)(j * 128), reinterpret_cast<const char*>(p.residual),
                                rs_wave + (unsigned)((mb & 1) * D_RUNIT + (j * 4 + rb) * 1024));
            }
        };
        auto read_block = [&](auto NB, auto MB, res_t (&t)[4]) {
            constexpr int nb = decltype(NB)::value, mb = decltype(MB)::value;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                t[g] = *reinterpret_cast<const u32x2*>(rs_rd + (mb & 1) * D_RUNIT + (nb >> 1) * 4096 + (rd_off ^ (unsigned)(((nb & 1) * 4 + g) << 4)));
        };
        // YOUNGER: the DMA pieces issued after this unit's (12 per unit still in flight behind it).  The reads of block nb + 1
        // are issued before block nb is converted.
        auto read_unit = [&](auto MB, auto YOUNGER) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(YOUNGER)::value) : "memory");
            if constexpr (decltype(MB)::value == 0) DITTO_BAR();   // every wave is past a wait that covers wave 0's bias row (the oldest load): visible to all
            res_t ta[4], tb[4];
            read_block(IntC<0>{}, MB, ta);
            read_block(IntC<1>{}, MB, tb); init_block(IntC<0>{}, MB, ta);
            read_block(IntC<2>{}, MB, ta); init_block(IntC<1>{}, MB, tb);
            read_block(IntC<3>{}, MB, tb); init_block(IntC<2>{}, MB, ta);
            read_block(IntC<4>{}, MB, ta); init_block(IntC<3>{}, MB, tb);
            read_block(IntC<5>{}, MB, tb); init_block(IntC<4>{}, MB, ta);
            init_block(IntC<5>{}, MB, tb);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the buffer is read: the next unit's DMA may overwrite it
        };
        issue_unit(IntC<0>{}); issue_unit(IntC<1>{});
        read_unit(IntC<0>{}, IntC<12>{}); issue_unit(IntC<2>{});
        read_unit(IntC<1>{}, IntC<12>{}); issue_unit(IntC<3>{});
        read_unit(IntC<2>{}, IntC<12>{});
        read_unit(IntC<3>{}, IntC<0>{});
    } else {
        // fp32 stream: 96 hand-written global_load_dwordx4 per lane in the accumulator layout, four 32 x 32 blocks (16 loads) in
        // flight.  (Round 5 A/B of a deeper window on the bf16 form of these loads, profiles/r05_frd_window_ab.txt: inside the
        // noise — the phase was bound by its 16-byte requests, not by the window.)
        const char* rp[4] = {nullptr, nullptr, nullptr, nullptr};
        if constexpr (RES && !HB) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                int gr = m0 + mb * 32 + r32;
                gr = gr < p.M ? gr : p.M - 1;
                rp[mb] = reinterpret_cast<const char*>(p.residual + (size_t)gr * p.ldr + wid * 192 + 4 * hh);
            }
        }
        constexpr int WD = 4, NG = 24;                               // window depth (groups of four loads in flight per wave); 24 groups = (nb, mb) blocks, mb fastest
        constexpr bool LOADS = RES && !HB && !FRD_NORES;
        res_t T[WD][4];
        auto issue_group = [&](auto GI, res_t (&t)[4]) {
            constexpr int nb = frd_group_nb(decltype(GI)::value), mb = frd_group_mb(decltype(GI)::value);
            if constexpr (LOADS) {
                fr_res_load<nb>(t, rp[mb]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = res_t{};
            }
        };
        auto finish_group = [&](auto GI, res_t (&t)[4]) {
            constexpr int gi = decltype(GI)::value, nb = frd_group_nb(gi), mb = frd_group_mb(gi);
            constexpr int younger = NG - 1 - gi < WD - 1 ? NG - 1 - gi : WD - 1;
            if constexpr (LOADS)
                fr_res_wait<4 * younger>(t);
            if constexpr (gi == 0) {
                if constexpr (!LOADS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                DITTO_BAR();      // every wave is past a wait that covers wave 0's bias row (the oldest load): visible to all
            }
            init_block(IntC<nb>{}, IntC<mb>{}, t);
        };
        auto init_step = [&](auto GI) {
            constexpr int gi = decltype(GI)::value;
            finish_group(GI, T[gi % WD]);
            if constexpr (gi + WD < NG) issue_group(IntC<gi + WD>{}, T[gi % WD]);
        };
        issue_group(IntC<0>{}, T[0]); issue_group(IntC<1>{}, T[1]); issue_group(IntC<2>{}, T[2]); issue_group(IntC<3>{}, T[3]);
        init_step(IntC<0>{}); init_step(IntC<1>{}); init_step(IntC<2>{}); init_step(IntC<3>{}); init_step(IntC<4>{}); init_step(IntC<5>{});
        init_step(IntC<6>{}); init_step(IntC<7>{}); init_step(IntC<8>{}); init_step(IntC<9>{}); init_step(IntC<10>{}); init_step(IntC<11>{});
        init_step(IntC<12>{}); init_step(IntC<13>{}); init_step(IntC<14>{}); init_step(IntC<15>{}); init_step(IntC<16>{}); init_step(IntC<17>{});
        init_step(IntC<18>{}); init_step(IntC<19>{}); init_step(IntC<20>{}); init_step(IntC<21>{}); init_step(IntC<22>{}); init_step(IntC<23>{});
    }

    // A slab 0 has landed for this wave (older than the residual loads); for everyone:
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    DITTO_BAR();
    FRD_STAMP(1);
    // W stages 0 and 1 -> the register ring (twelve loads, nothing else behind them: the wait counts of frd_vm start here)
    issue_w(IntC<0>{}, wr[0][0]); issue_w(IntC<1>{}, wr[0][1]); issue_w(IntC<2>{}, wr[0][2]);
    issue_w(IntC<3>{}, wr[0][3]); issue_w(IntC<4>{}, wr[0][4]); issue_w(IntC<5>{}, wr[0][5]);
    advance_w();
    issue_w(IntC<0>{}, wr[1][0]); issue_w(IntC<1>{}, wr[1][1]); issue_w(IntC<2>{}, wr[1][2]);
    issue_w(IntC<3>{}, wr[1][3]); issue_w(IntC<4>{}, wr[1][4]); issue_w(IntC<5>{}, wr[1][5]);
    advance_w();
    unsigned a_cur = 0;          // byte offset of the A slab being multiplied
    bf16x8 a0[4], a1[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) a0[mb] = *reinterpret_cast<const bf16x8*>(smem + a_cur + a_row + mb * 4096 + a_x);

    // One stage = K 16 at slab position J.  LAST: the last slab (no next slab to fetch; its stages 2, 3 fetch no W).
    // ACUR: this stage's A fragments (resident), ANXT receives the next stage's.
    auto stage = [&](auto J, auto LAST, bf16x8 (&ACUR)[4], bf16x8 (&ANXT)[4]) {
        constexpr int j = decltype(J)::value;
        constexpr bool last = decltype(LAST)::value != 0;
        constexpr bool do_w = !(last && j >= 2), do_a = !last && j < 2, has_next = !(last && j == 3);
        constexpr int slot = j & 1;
        const unsigned a_nxt = j == 3 ? (unsigned)D_ASLAB - a_cur : a_cur;
#pragma unroll
        for (int nb = 0; nb < 6; ++nb) {
            if (nb == 4 && has_next) {
                if constexpr (j == 3) {
                    // the next slab: this wave's four pieces have landed (issued at j = 0, 1; 6 + 4 loads since), everyone's
                    // behind the barrier, which also certifies that every wave is done reading the slab the NEXT issue overwrites
                    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
#ifndef DITTO_DIAG_FR_NOBAR
                    DITTO_BAR();
#endif
                }
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
                    ANXT[mb] = *reinterpret_cast<const bf16x8*>(smem + a_nxt + a_row + mb * 4096 + (a_x ^ (((j + 1) & 3) << 5)));
            }
            // fragment (s, nb) has landed: everything but the frd_vm(j, nb) operations issued after it
            if (nb == 0) wait_frag(IntC<frd_vm(j, 0, last)>{}, wr[slot][0]);
            if (nb == 1) wait_frag(IntC<frd_vm(j, 1, last)>{}, wr[slot][1]);
            if (nb == 2) wait_frag(IntC<frd_vm(j, 2, last)>{}, wr[slot][2]);
            if (nb == 3) wait_frag(IntC<frd_vm(j, 3, last)>{}, wr[slot][3]);
            if (nb == 4) wait_frag(IntC<frd_vm(j, 4, last)>{}, wr[slot][4]);
            if (nb == 5) wait_frag(IntC<frd_vm(j, 5, last)>{}, wr[slot][5]);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                if constexpr (has_next) {
                    if (nb < DNA) fr_mfma(InAgpr{}, acca[nb < DNA ? nb : 0][mb], wr[slot][nb], ACUR[mb]);
                    else fr_mfma(InVgpr{}, accv[nb < DNA ? 0 : nb - DNA][mb], wr[slot][nb], ACUR[mb]);
                } else {
                    if (nb < DNA) fr_mfma_last(InAgpr{}, acca[nb < DNA ? nb : 0][mb], wr[slot][nb], ACUR[mb]);
                    else fr_mfma_last(InVgpr{}, accv[nb < DNA ? 0 : nb - DNA][mb], wr[slot][nb], ACUR[mb]);
                }
            }
            if constexpr (do_w) {   // fragment nb of stage s + 2 into the registers just consumed
                if (nb == 0) issue_w(IntC<0>{}, wr[slot][0]);
                if (nb == 1) issue_w(IntC<1>{}, wr[slot][1]);
                if (nb == 2) issue_w(IntC<2>{}, wr[slot][2]);
                if (nb == 3) issue_w(IntC<3>{}, wr[slot][3]);
                if (nb == 4) issue_w(IntC<4>{}, wr[slot][4]);
                if (nb == 5) issue_w(IntC<5>{}, wr[slot][5]);
            }
            if constexpr (do_a) {   // half of the next slab's four pieces, behind W4 and W5
                if (nb == 4) issue_a_piece(IntC<2 * j>{});
                if (nb == 5) issue_a_piece(IntC<2 * j + 1>{});
            }
        }
        if constexpr (do_w) advance_w();
        if constexpr (do_a && j == 1) advance_a();
        if constexpr (j == 3) a_cur = a_nxt;
    };
    for (int sl = 0; sl + 1 < nslab; ++sl) {
        stage(IntC<0>{}, IntC<0>{}, a0, a1);
        stage(IntC<1>{}, IntC<0>{}, a1, a0);
        stage(IntC<2>{}, IntC<0>{}, a0, a1);
        stage(IntC<3>{}, IntC<0>{}, a1, a0);
    }
    stage(IntC<0>{}, IntC<1>{}, a0, a1);
    stage(IntC<1>{}, IntC<1>{}, a1, a0);
    stage(IntC<2>{}, IntC<1>{}, a0, a1);
    stage(IntC<3>{}, IntC<1>{}, a1, a0);

    // ---------------- epilogue: the accumulators hold h = residual + bias + A W^T; they are only READ from here on ----------------
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    DITTO_BAR();                                                       // every wave is out of the main loop: the A slabs are idle
    FRD_STAMP(2);
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, rstd[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (LN) {
        if (wid < 2) {   // gamma and beta rows -> LDS (3 pieces of 1 KiB each), landed by the first exchange below
            const float* src = wid == 0 ? fp.gamma : fp.beta;
#pragma unroll
            for (int i = 0; i < 3; ++i) glds16(src + i * 256 + lane * 4, lds_base + (unsigned)(D_GB + wid * DN * 4 + i * 1024));
        }
        // Row statistics, two passes like nn.LayerNorm: per lane one chain over this wave's quarter row, + lane ^ 32, then
        // (q0 + q1) + (q2 + q3) through LDS.  The fused forms are written out (contraction would follow basic-block structure).
        float rsum[4] = {0.f, 0.f, 0.f, 0.f};
        float* red = reinterpret_cast<float*>(smem + D_RED);         // [quarter][128 rows]
        auto row_pass = [&](auto PASS, float (&c4)[4]) {
#pragma unroll
            for (int nb = 0; nb < 6; ++nb)
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
                    // re-pin the block in its home file: the copy below is then a NEW value that cannot be hoisted above this (fr_common.h fr_pin)
                    if (nb < DNA) fr_pin(InAgpr{}, acca[nb < DNA ? nb : 0][mb]); else fr_pin(InVgpr{}, accv[nb < DNA ? 0 : nb - DNA][mb]);
                    const f32x16 v = nb < DNA ? acca[nb < DNA ? nb : 0][mb] : accv[nb < DNA ? 0 : nb - DNA][mb];
                    fr_row_acc<decltype(PASS)::value, DN>(c4[mb], v, rsum[mb]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                float t = c4[mb];
                t += __shfl_xor(t, 32, 64);
                if (hh == 0) red[wid * DM + mb * 32 + r32] = t;
            }
        };
        float c4[4] = {0.f, 0.f, 0.f, 0.f};
        row_pass(IntC<0>{}, c4);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // gamma / beta have landed
        __syncthreads();
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const int r = mb * 32 + r32;
            rsum[mb] = (red[r] + red[DM + r]) + (red[2 * DM + r] + red[3 * DM + r]);
            mean[mb] = rsum[mb] * (1.0f / DN);
            asm volatile("" : "+v"(mean[mb]));                        // the ROUNDED mean, never re-fused into a consumer
        }
        __syncthreads();                                              // everyone has read the sums before the next pass overwrites them
        float q4[4] = {0.f, 0.f, 0.f, 0.f};
        row_pass(IntC<1>{}, q4);
        __syncthreads();
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const int r = mb * 32 + r32;
            rstd[mb] = rsqrtf(fmaf((red[r] + red[DM + r]) + (red[2 * DM + r] + red[3 * DM + r]), 1.0f / DN, 1e-5f));
        }
    }
    FRD_STAMP(3);
    // stores: every output row leaves through a wave-private LDS stage so that the stores are whole 128-B lines:
    // h fp32 (nt), u = LN(h) bf16, optional bf16 copy of h.
    const int cl = wid * 192 + 4 * hh;                             // this lane's column origin; + nb * 32 + 8 g
    const float* gl = lgamma + cl;
    const float* bl = lbeta + cl;
    char* hst = smem + wid * 32768;                                 // h stage: [128 rows][128 B]
    char* ust = hst + 16384;                                        // u stage: [128 rows][128 B] = 64 bf16 columns
    const int srow = lane >> 3, sq = lane & 7;                      // read-back: row srow (+ 8 i), 16-B chunk sq
    const int grow0 = m0 + srow;
    float* hrow = (float*)p.out + (size_t)(grow0 < p.M ? grow0 : 0) * p.ldo + wid * 192 + sq * 4;
    bf16* hbrow = (bf16*)p.out + (size_t)(grow0 < p.M ? grow0 : 0) * p.ldo + wid * 192 + sq * 8;   // HB
    bf16* urow = fp.u ? fp.u + (size_t)(grow0 < p.M ? grow0 : 0) * fp.ldu + wid * 192 + sq * 8 : nullptr;
    bf16* orow = p.out2 ? p.out2 + (size_t)(grow0 < p.M ? grow0 : 0) * p.ldo2 + wid * 192 + sq * 8 : nullptr;
#pragma unroll
    for (int nb = 0; nb < 6; ++nb) {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            if (nb < DNA) fr_pin(InAgpr{}, acca[nb < DNA ? nb : 0][mb]); else fr_pin(InVgpr{}, accv[nb < DNA ? 0 : nb - DNA][mb]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = nb * 32 + 8 * g;                         // compile-time
            f32x4 g4 = {1.f, 1.f, 1.f, 1.f}, b4 = {0.f, 0.f, 0.f, 0.f};
            if constexpr (LN) {
                g4 = *reinterpret_cast<const f32x4*>(gl + co);
                b4 = *reinterpret_cast<const f32x4*>(bl + co);
            }
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                const f32x16& v = nb < DNA ? acca[nb < DNA ? nb : 0][mb] : accv[nb < DNA ? 0 : nb - DNA][mb];
                const f32x4 v4 = {v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
                const int row = mb * 32 + r32;
                if constexpr (HB) {                                  // h as bf16: the same [128 rows][64 columns] image as u
                    u32x2 sh;
                    sh[0] = pack_bf16x2(v4[0], v4[1]); sh[1] = pack_bf16x2(v4[2], v4[3]);
                    *reinterpret_cast<u32x2*>(hst + row * 128 + ((((nb & 1) * 4 + g) ^ (row & 7)) << 4) + hh * 8) = sh;
                } else {
                    fr_stage_f32(hst, row, g, hh, v4);
                }
                if constexpr (LN || !HB) {
                    f32x4 y = v4;                                    // bf16 side: LayerNorm output, or the plain copy
                    if constexpr (LN) y = (v4 - mean[mb]) * rstd[mb] * g4 + b4;
                    fr_stage_bf16(ust, row, nb, g, hh, y);
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (!HB) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int i = 4 * q; i < 4 * q + 4; ++i) {
                    const int row = srow + 8 * i;
                    const u32x4 hv = *reinterpret_cast<const u32x4*>(hst + row * 128 + ((sq ^ (row & 7)) << 4));
                    if (grow0 + 8 * i < fr_store_m(p)) store16<true, true>(hrow + (size_t)(8 * i) * p.ldo + nb * 32, hv, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else if (nb & 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int i = 4 * q; i < 4 * q + 4; ++i) {
                    const int row = srow + 8 * i;
                    const u32x4 hv = *reinterpret_cast<const u32x4*>(hst + row * 128 + ((sq ^ (row & 7)) << 4));
                    if (grow0 + 8 * i < fr_store_m(p)) *reinterpret_cast<u32x4*>(hbrow + (size_t)(8 * i) * p.ldo + (nb - 1) * 32) = hv;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if ((nb & 1) && (LN || !HB)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int i = 4 * q; i < 4 * q + 4; ++i) {
                    const int row = srow + 8 * i;
                    const u32x4 uv = *reinterpret_cast<const u32x4*>(ust + row * 128 + ((sq ^ (row & 7)) << 4));
                    if (grow0 + 8 * i < fr_store_m(p)) {
                        if (LN) *reinterpret_cast<u32x4*>(urow + (size_t)(8 * i) * fp.ldu + (nb - 1) * 32) = uv;
                        else if (orow) *reinterpret_cast<u32x4*>(orow + (size_t)(8 * i) * p.ldo2 + (nb - 1) * 32) = uv;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
#ifdef DITTO_DIAG_FRD_STAMP
    {
        FRD_STAMP(4);                                                // (stores issued)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        FRD_STAMP(5);                                                // (stores drained)
        const int w = blockIdx.x * 4 + wid;
#ifdef DITTO_DIAG_FRD_STAMP_K   // record only the launches of this depth WITH a LayerNorm (in-model stamps: tools/frd_stamps_model.py)
        if (p.K == DITTO_DIAG_FRD_STAMP_K && LN)
#endif
        if (lane == 0 && w < 1024 * 4) {
            g_frd_stamps[w * 8 + 0] = frd_t1 - frd_t0; g_frd_stamps[w * 8 + 1] = frd_t2 - frd_t1; g_frd_stamps[w * 8 + 2] = frd_t3 - frd_t2;
            g_frd_stamps[w * 8 + 3] = frd_t4 - frd_t3; g_frd_stamps[w * 8 + 4] = frd_t5 - frd_t4; g_frd_stamps[w * 8 + 5] = 1;
        }
    }
#endif
}

template <bool LN, bool RES, bool HB = false>
hipError_t launch_frd_t(const FrParams& fp, int grid, hipStream_t s) {
    static DevOnce lds_once;
    if (hipError_t e = set_max_lds_once(lds_once, {reinterpret_cast<const void*>(&gemm_frd_kernel<LN, RES, HB>)}, D_LDS)) return e;
    hipLaunchKernelGGL((gemm_frd_kernel<LN, RES, HB>), dim3(grid), dim3(256), D_LDS, s, fp);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gemm_frd(const FrParams& fp_in, hipStream_t s) {
    FrParams fp = fp_in;
    if (fp.g.N != DN || fp.u_fp8) return hipErrorInvalidValue;
    fp.g.tiles_m = (fp.g.M + DM - 1) / DM;
    fp.g.tiles_n = 1;
    const bool ln = fp.gamma && fp.u, res = fp.g.residual != nullptr;
    // the bf16 residual tile is fetched by 16-byte LDS-DMA pieces at 32-bit byte offsets from the residual pointer
    if (fp.hb && res && (fp.g.ldr % 8 || (uintptr_t)fp.g.residual % 16 || (size_t)fp.g.M * (size_t)fp.g.ldr * 2 >= (1ull << 32)))
        return hipErrorInvalidValue;
    if (fp.hb) {   // bf16 residual stream (the model path's two launches: always with a residual), or — no residual, no LayerNorm —
                   // a plain product with a bf16 result (the training backward's long-K dgrads)
        if (fp.g.out2 || (!res && ln)) return hipErrorInvalidValue;
        if (!res) return launch_frd_t<false, false, true>(fp, fp.g.tiles_m, s);
        return ln ? launch_frd_t<true, true, true>(fp, fp.g.tiles_m, s) : launch_frd_t<false, true, true>(fp, fp.g.tiles_m, s);
    }
    if (ln) return res ? launch_frd_t<true, true>(fp, fp.g.tiles_m, s) : launch_frd_t<true, false>(fp, fp.g.tiles_m, s);
    return res ? launch_frd_t<false, true>(fp, fp.g.tiles_m, s) : launch_frd_t<false, false>(fp, fp.g.tiles_m, s);
}

#ifdef DITTO_DIAG_FRD_STAMP
}  // namespace ditto
extern "C" int ditto_diag_frd_stamps(unsigned long long* out, int n) {   // raw per-wave records of the LAST launch (diagnostic build only)
    if (n > 1024 * 4 * 8) n = 1024 * 4 * 8;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ditto::g_frd_stamps), (size_t)n * 8) != hipSuccess;
}
namespace ditto {
#endif

}  // namespace ditto
