// forward_plan.hip — which kernel class the launches of one forward take (model.h ForwardPlan): host arithmetic on the config, the
// rows, the split-K scratch size and the calling thread's options, no HIP call.  An utterance's bits depend on this class and on
// nothing else, so it is decided HERE, once per call; every launch site only reads the plan.
#include <cstdlib>

#include "gemm_common.h"
#include "model.h"

namespace ditto {

// Small batches leave the long-K GEMMs of the step on a few dozen workgroups, each walking all of K alone (B = 1: fc2 is 48 tiles x
// 48 K-tiles = 41 us for 4.8 GFLOP).  Those run split-K: `splits` workgroups per output tile write fp32 partials, launch_splitk_finish
// adds them in order together with bias and residual.  "splitk_wgs" > 0 (DITTO_SPLITK_WGS): a target of that many workgroups in
// flight, at least 4 K-tiles per split (tools/step_ab.py, C2 at 256: B = 1 fc2 40.6 -> 24.2 us, step 1.87 -> 1.68 ms; B >= 4 never
// splits) — that K-partition depends on the batch size, so with it an utterance's result is no longer bit-identical across batch
// compositions, the property tests/test_gpu_model.py::test_full_size_c2_properties holds the default (0) to.
int g_splitk_wgs = [] { const char* e = getenv("DITTO_SPLITK_WGS"); return e ? atoi(e) : 0; }();
// "residual_bf16": the residual stream h between the segments of a block lives in HBM as bf16 (fp32 only inside accumulators
// and LayerNorm statistics) wherever the launch takes the full-row class at d = 768 / head_dim 64 (plan_forward decides)
// "ll_mask": the low-latency class's launch forms: bit 0 = fc2's split-K finish also writes the NEXT block's norm1 (no bit changes),
// bit 1 = the cross out-projection runs as two K-splits whose finish also writes norm3 (that GEMM's summation order: part of the class)
int g_ll_mask = [] { const char* e = getenv("DITTO_LL_MASK"); const int v = e ? atoi(e) : 3; return v < 0 || v > 3 ? 3 : v; }();
// "lnq": norm2 fused into the cross-attention q-projection (gemm_lnq.hip) for launches of the full-row class at d = 768:
// 0 = off (LayerNorm launch + tiled GEMM), 32 / 16 = on, with that MFMA shape (32x32x16 / 16x16x32)
// "lnq_min_rows": > 0: the fused norm2 + q-projection also runs BELOW the full-row class, from that many (class) rows on (A/B)
// Default 8192 since round 5: with the kernel on two waves per SIMD the fused launch wins from 128 of its 64-row tiles on
// (profiles/r05_small_batch_lnq8.txt, same process: B = 8 4.02 -> 3.95 ms, B = 16 6.63 -> 6.47; B = 4 2.61 -> 2.63, hence not lower).
int g_lnq_min_rows = [] { const char* e = getenv("DITTO_LNQ_MIN_ROWS"); return e ? atoi(e) : 8192; }();
int g_lnq = [] { const char* e = getenv("DITTO_LNQ"); const int v = e ? atoi(e) : 32; return v == 0 || v == 16 || v == 32 ? v : 32; }();   // validated like ditto_set_option
int g_resid_bf16 = [] { const char* e = getenv("DITTO_RESIDUAL_BF16"); return e ? (atoi(e) != 0) : 1; }();   // normalised to 0 / 1
// "qkv_split" (round 5): 0 = off; n > 0 = the QKV GEMM's last 256 columns as a second launch where that leaves whole rounds of
// 256 x 256 tiles (plan_forward), for launches of at most n rounds of such tiles.  Default 3 = B = 8 and B = 16 at N = 1024
// (profiles/r05_qkv_split_ab.txt, same process: QKV 48.6 -> 44.4 us / 75.6 -> 72.3, step 3.87 -> 3.83 / 6.44 -> 6.42 ms; B = 24 and
// B = 32 — 3.4 and 4.5 rounds — do not gain: the small-tile tail launch costs what the half round did).  Bit-identical either way.
int g_qkv_split = [] { const char* e = getenv("DITTO_QKV_SPLIT"); return e ? atoi(e) : 3; }();
static int small_batch_k_splits(int M, int N, int K) {
    if (g_splitk_wgs < 0) return 1;                        // -1: never split
    const int ktiles = K / 64;
    if (g_splitk_wgs == 0) {
        // Default since round 4: the LOW-LATENCY CLASS.  A batch of at most 2048 rows (1-2 utterances at N = 1024: the reference's
        // own call pattern, Experiments.ipynb:125-132) leaves its long-K GEMMs (fc2: 48 tiles x 48 K-tiles at B = 1; the final
        // projection) on a fifth of the chip; they run split over K with an ordered fp32 reduce (bias + residual in the reduce):
        // fc2 40.8 -> 24.2 us, step 1.83 -> 1.63 ms at C2 B = 1.  The number of splits depends on K ONLY, so inside the class an
        // utterance's bits do not depend on its batch neighbours; the class is pinnable like the full-row one (kernels.h fr_rule_rows).
        if (class_rows(M) > 2048 || ktiles < 24) return 1;
        return ktiles / 12 > 8 ? 8 : ktiles / 12;          // K = 3072: 4, 1536: 2, 4096: 5, 2048: 2
    }
    const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);   // > 0: the explicit rule of rounds 1-3 (a workgroup target)
    if (tiles > 256 || ktiles < 16) return 1;
    long ns = g_splitk_wgs / tiles;
    if (ns > ktiles / 4) ns = ktiles / 4;
    if (ns > 8) ns = 8;
    return ns < 2 ? 1 : (int)ns;
}

// The cross out-projection (K = d) in the low-latency class: two K-splits (its 48 tiles at B = 1 become 96 workgroups of half the
// depth) whose finish also writes norm3 — the LayerNorm launch behind it disappears.  Same class rule as above, K only.
static int small_batch_k_splits_outproj(int M, int K) {
    return (g_splitk_wgs == 0 && (g_ll_mask & 2) && class_rows(M) <= 2048 && K / 64 >= 12) ? 2 : 1;
}

// The plan of a forward over M rows whose split-K scratch holds `splitk_bytes`.  Every rule is judged on the CLASS rows
// (kernels.h class_rows) unless said otherwise.  Where the askers have always differed, `who` keeps the difference:
//   - the pinned class below 64 rows: an error for every asker but PLAN_TRAIN, which never checked it
//   - fr_out / fr_fc2: PLAN_TRAIN has them at d = 768 only, and only with both weight copies
//   - the bf16 stream.  PLAN_FORWARD, PLAN_QUERY: "residual_bf16", and the 128-row kernel by fr_tile 130 or by the rule on the class
//     rows.  PLAN_TRAIN: not "residual_bf16" but train_flags 8 | 16 and attn_flags 8192 off, and BOTH launches on the 128-row kernel
//     by fr_launch_kernel (which differs under fr_tile 64 with a small fr64_maxk).  Both need fr_mask 3 (= fr_out and fr_fc2).
//     PLAN_BLOCK: a lone block has the fp32 stream
//   - that stream's class at M < 128 (only gemm_frd.hip has the bf16 form; a pinned class would run the 64-row kernel): an error
//     for PLAN_FORWARD, hb = false for PLAN_QUERY; PLAN_TRAIN's test is false there by itself
//   - q_split is judged on the launch's OWN M and on gemm_tile 0: it changes no bit
//   - fc2's and the out-projection's K-splits are off with fp8 linears; the final projection's (a bf16 GEMM there too) are not.
//     Every K-split needs the scratch to hold its partials, and with it chain_ll, which needs ns_fc2 of them
//   - the norm1 chain is PLAN_FORWARD's and PLAN_QUERY's: a lone block has no neighbours, PLAN_TRAIN reads fr_out, fr_fc2 and hb only
int plan_forward(const ditto_config& c, int M, size_t splitk_bytes, PlanFor who, ForwardPlan* out) {
    const int d = c.hidden_dim, dh = d / c.num_heads, dp = cfg_dp(c);
    const bool fp8 = (c.flags & DITTO_CFG_FP8_LINEAR) != 0, train = who == PLAN_TRAIN, whole = who == PLAN_FORWARD || who == PLAN_QUERY;
    const StagePacks have = stage_packs(c);   // the stage-major weight copies exist exactly where a kernel exists
    // A pinned kernel class (fr_class_rows > 0: "decide as the unsplit batch of that many rows would") that says full-row while THIS
    // launch cannot run a full-row kernel (fewer rows than one 64-row tile) would silently take the tiled GEMMs, whose last bits
    // differ: the promise of the pin — sharding changes no bit — would be broken without a sign.  Fail instead.
    if (!train && have.o && opt_class_rows() > 0 && opt_fr_mask() && M < 64 && (d == 1024 ? fr_pays_64(M) : fr_pays(M)))
        return fail(DITTO_ERR_SHAPE, "kernel class pinned to a batch of %d rows (full-row GEMM + LayerNorm kernels), but this launch has "
                                     "%d rows, fewer than one 64-row tile: it cannot take that class and its bits would differ from the "
                                     "unsplit batch's.  Give every shard at least 64 rows, or run the whole batch unfused "
                                     "(ditto_set_option(\"fr_mask\", 0)).", opt_class_rows(), M);
    ForwardPlan& p = *out = ForwardPlan{};
    p.fr_out = have.o && (!train || (d == 768 && have.fc2)) && (opt_fr_mask() & 1) && fr_outproj_ok(M, d);
    p.fr_fc2 = have.fc2 && (!train || (d == 768 && have.o)) && (opt_fr_mask() & 2) && fr_fc2_ok(M, d);
    // bf16 residual stream: only where EVERY consumer of h has the bf16 form — d = 768, head_dim 64, both fused launches on gemm_frd.hip
    const bool both = p.fr_out && p.fr_fc2 && d == 768 && dh == 64;
    if (train) p.hb = both && !(g_train_flags & (8 | 16)) && !(g_attn_flags & 8192) && fr_launch_kernel(M, d) == 130 && fr_launch_kernel(M, 4 * d) == 130;
    else if (whole) {
        p.hb = both && opt_resid_bf16() && (g_fr_tile == 130 || (g_fr_tile == 0 && fr_rule_rows(class_rows(M)) == 130));
        if (p.hb && M < 128 && who == PLAN_FORWARD)
            return fail(DITTO_ERR_SHAPE, "kernel class pinned to a batch of %d rows (bf16 residual stream on the 128-row full-row kernel), "
                                         "but this launch has %d rows: it cannot take that class.  Give every shard at least 128 rows, or "
                                         "ditto_set_option(\"residual_bf16\", 0).", opt_class_rows(), M);
        p.hb = p.hb && M >= 128;
    }
    // "lnq" (d = 1024, BASELINE config C5: the same kernel at that width, 32x32x16 only, by the rule of its full-row GEMM)
    if (opt_lnq() && have.lnq && (d == 768 ? fr_pays(M) || (g_lnq_min_rows > 0 && class_rows(M) >= g_lnq_min_rows) : fr_pays_64(M)))
        p.lnq = d == 768 ? opt_lnq() : 32;
    // "qkv_split": a fractional round of 256 x 256 tiles, whole rounds without the LAST 256 columns (d = 768, B = 8: 288 tiles = 1.125 rounds)
    const long q_tm = (M + 255) / 256, q_tn = (3 * dp) / 256;
    p.q_split = g_qkv_split && !fp8 && dh == 64 && g_gemm_tile == 0 && (3 * dp) % 256 == 0 && 3 * dp >= 2048 + 256 &&
                2 * d <= 3 * dp - 256 && q_tm * q_tn >= 144 && (q_tm * q_tn) % 256 != 0 && (q_tm * (q_tn - 1)) % 256 == 0 &&
                q_tm * q_tn <= (long)g_qkv_split * 256;
    auto fits = [&](int ns) { return ns > 1 && splitk_bytes >= (size_t)ns * M * d * 4 ? ns : 1; };
    p.ns_out = (fp8 || p.fr_out) ? 1 : fits(small_batch_k_splits_outproj(M, dp));
    p.ns_fc2 = (fp8 || p.fr_fc2) ? 1 : fits(small_batch_k_splits(M, d, 4 * d));
    p.ns_fin = fits(small_batch_k_splits(M, d, 2 * d));
    // fc2 on the full-row kernel also emits the NEXT block's norm1; in the low-latency class fc2's split-K finish does (ll_mask bit 0);
    // block 0's rides in the GlobalAdaLN kernel (gemm_flags bit 15: A/B off).  Each in the LayerNorm kernel's statistics order: the same bits
    p.chain_ln1 = whole && p.fr_fc2;
    p.chain_ll = whole && !p.fr_fc2 && (g_ll_mask & 1) && p.ns_fc2 > 1;
    p.ln1_in_adaln = whole && !fp8 && !(g_gemm_flags & 32768);
    return DITTO_OK;
}

}  // namespace ditto
