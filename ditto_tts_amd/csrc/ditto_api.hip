// ditto_api.hip — the C-ABI of libditto_hip.so (include/ditto_hip.h): model handle, weight packing,
// the stream-ordered launch sequence of one DiTTO.forward, the sampler update.
//
// HBM layout (one contiguous caller-owned arena per model, one workspace per (B,N,T), one cond buffer
// per utterance batch).  All offsets 256-byte aligned.
//   arena     : per layer { Wqkv bf16[3d,d] | Wcq bf16[d,d] | Wco bf16[d,d] | W1g bf16[8d,d] (fc1/gate rows
//               interleaved in blocks of 16) | W2 bf16[d,4d] | biases + LN gamma/beta fp32 },
//               Wkv_all bf16[L*2d, d] (cross-attn K,V projections of every layer), Wfin bf16[d, 2d]
//               ([proj_in | proj_out] along K), time table fp32[steps, 2d], text_mlp fp32, inv_freq.
//   cond      : kv_cache bf16[B*T, L*2d] (layer l: K at cols l*2d.., V at l*2d+d..) | tmod fp32[B, 2d]
//   workspace : h fp32[M,d] (residual stream) | u bf16[M,d] | qkv bf16[M,3d] | act bf16[M,4d] |
//               xcat bf16[M,2d] ([bf16(x_raw) | bf16(h_L)]) | eps fp32[M,d] | attention scratch
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <new>
#include <vector>

#include "batch_layout.h"
#include "ditto_project.h"
#include "ditto_project_stream.h"
#include "ditto_refresh.h"
#include "gemm_common.h"

using namespace ditto;

namespace ditto {
extern thread_local int t_gemm_structure;   // gemm.hip: the tile structure this thread's last launch_gemm took (ditto_gemm_epilogue_bf16)

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

ArenaPlan plan_arena(const ditto_config& c) {
    ArenaPlan p;
    const size_t d = c.hidden_dim, L = c.num_layers;
    const size_t dp = cfg_dp(c);                                      // attention-side width (= d unless heads are padded)
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    p.layers.resize(L);
    for (size_t l = 0; l < L; ++l) {
        auto& q = p.layers[l];
        const size_t we = (c.flags & DITTO_CFG_FP8_LINEAR) ? 1 : 2;   // bytes per element of the fp8-able weights
        q.Wqkv = take(3 * dp * d * we); q.Wcq = take(dp * d * 2); q.Wco = take(d * dp * 2);
        q.W1g = take(8 * d * d * we); q.W2 = take(4 * d * d * we);
        q.sqkv = take(3 * dp * 4); q.s1g = take(8 * d * 4); q.s2 = take(d * 4);   // fp8 per-row weight scales
        q.bqkv = take(3 * dp * 4); q.bcq = take(dp * 4); q.bco = take(d * 4); q.b1g = take(8 * d * 4); q.b2 = take(d * 4);
        q.g1 = take(d * 4); q.be1 = take(d * 4); q.g2 = take(d * 4); q.be2 = take(d * 4); q.g3 = take(d * 4);
        q.be3 = take(d * 4);
        // stage-major bf16 copies of the N = d projections for the full-row kernels (gemm_fr.hip, gemm_fr64.hip) and of the cross
        // q-projection for the fused norm2 + q-projection kernel (gemm_lnq.hip; d == 768: both MFMA shapes' images): model.h stage_packs
        const StagePacks have = stage_packs(c);
        q.WcoP = have.o ? take(d * d * 2) : 0; q.W2P = have.fc2 ? take(4 * d * d * 2) : 0;
        q.WcqP = have.lnq ? take(d * d * 2) : 0; q.WcqP32 = have.lnq && d == 768 ? take(d * d * 2) : 0;
    }
    p.Wkv = take(L * 2 * dp * d * 2); p.bkv = take(L * 2 * dp * 4);
    p.Wfin = take(d * 2 * d * 2); p.bfin = take(d * 4);
    p.ttab = take((size_t)c.diffusion_steps * 2 * d * 4);
    p.wx = take(2 * d * (size_t)c.text_dim * 4); p.bx = take(2 * d * 4);
    p.invf = take((d / c.num_heads / 2) * 4);
    p.invf_rev = take((d / c.num_heads / 2) * 4);
    p.total = off;
    return p;
}

// ditto_text_precompute scratch (front of the same workspace) over `rows` text rows of B utterances: bf16(text) | pooled fp32
static inline size_t text_scratch_bytes(const ditto_config& c, int B, size_t rows) {
    return al(rows * c.text_dim * 2) + al((size_t)B * c.text_dim * 4);
}

WsPlan plan_ws(const ditto_config& c, int B, int N, int T) {
    WsPlan w;
    const size_t d = c.hidden_dim, M = (size_t)B * N, dh = cfg_dhp(c), dp = cfg_dp(c);   // dh: the PHYSICAL head width
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    w.h = take(M * d * 4); w.u = take(M * dp * 2); w.qkv = take(M * 3 * dp * 2); w.act = take(M * 4 * d * 2);
    w.xcat = take(M * 2 * d * 2); w.eps = take(M * d * 4);
    const size_t a1 = attention_workspace_bytes(B, c.num_heads, N, N, (int)dh);
    const size_t a2 = attention_workspace_bytes(B, c.num_heads, N, T, (int)dh);
    w.attn_bytes = a1 > a2 ? a1 : a2;
    w.attn = take(w.attn_bytes);
    // split-K partials of fc2 / the final projection at small batch: sized for the most splits the option allows
    w.splitk_bytes = (long)((M + 127) / 128) * ((d + 127) / 128) <= 256 ? 8 * M * d * 4 : 0;
    w.splitk = take(w.splitk_bytes);
    w.utt = w.pos = 0;
    const size_t tneed = text_scratch_bytes(c, B, (size_t)B * T);
    w.total = off > tneed ? off : tneed;
    return w;
}

// the workspace of a packed forward: plan_ws over the rows rounded up to whole 256-row tiles, then the two int32 row maps; the text
// precompute's scratch (bf16 text [S_T, dt] | pooled fp32 [B, dt]) at the front
static WsPlan plan_ws_packed(const ditto_config& c, int B, int S, int S_T) {
    WsPlan w = plan_ws(c, 1, (S + 255) / 256 * 256, S_T);
    size_t off = w.total;
    w.utt = off; off += al((size_t)S * 4);
    w.pos = off; off += al((size_t)S * 4);
    const size_t tneed = text_scratch_bytes(c, B, (size_t)S_T);
    w.total = off > tneed ? off : tneed;
    return w;
}

// (a step entry sizes its workspace before the forward has validated Mt)
WsPlan BatchLayout::plan(const ditto_config& c) const {
    return kind == PACKED ? plan_ws_packed(c, B, M, Mt > 0 ? Mt : 1) : plan_ws(c, B, N, T);
}

int check_cfg(const ditto_config* c) {
    if (!c) return fail(DITTO_ERR_ARG, "config is null");
    if (c->hidden_dim <= 0 || c->num_layers <= 0 || c->num_heads <= 0 || c->time_dim <= 0 || c->diffusion_steps <= 0)
        return fail(DITTO_ERR_SHAPE, "non-positive config field");
    if (c->hidden_dim % c->num_heads) return fail(DITTO_ERR_SHAPE, "hidden_dim %% num_heads != 0");
    if (c->text_dim != c->hidden_dim)
        return fail(DITTO_ERR_SHAPE, "text_dim (%d) must equal hidden_dim (%d): reference cross-attn has no kdim/vdim",
                    c->text_dim, c->hidden_dim);
    if (c->hidden_dim % 64) return fail(DITTO_ERR_SHAPE, "hidden_dim must be a multiple of 64 (MFMA K tile)");
    if (c->hidden_dim > 2048) return fail(DITTO_ERR_SHAPE, "hidden_dim > 2048 not supported by the LayerNorm kernel");
    const int dh = c->hidden_dim / c->num_heads;
    if (dh % 2) return fail(DITTO_ERR_SHAPE, "head_dim (%d) must be even (half-split RoPE, src/components/DiT.py:52-54)", dh);
    // head_dim % 64 != 0 (the reference takes any hidden_dim % num_heads == 0, src/components/DiT.py:78-86; e.g. 1152 / 16 = 72)
    // runs with the heads PADDED to the next multiple of 64 inside the block (model.h cfg_dhp): inference only, bf16 linears
    if (dh % 64 && (c->flags & DITTO_CFG_FP8_LINEAR))
        return fail(DITTO_ERR_SHAPE, "fp8 linear layers need head_dim %% 64 == 0 (head_dim %d)", dh);
    if (dh % 64 && 4 * c->hidden_dim < cfg_dp(*c))
        return fail(DITTO_ERR_SHAPE, "head_dim %d pads to %d: more than 4x hidden_dim of attention width is not supported", dh, cfg_dhp(*c));
    if ((c->flags & DITTO_CFG_FP8_LINEAR) && c->hidden_dim % 128)
        return fail(DITTO_ERR_SHAPE, "fp8 linear layers need hidden_dim %% 128 == 0");
    if (c->flags & ~DITTO_CFG_FP8_LINEAR) return fail(DITTO_ERR_ARG, "unknown config flag");
    return DITTO_OK;
}

int check_call_opts(const ditto_call_opts* o) {
    if (!o) return DITTO_OK;
    if (o->class_rows < -1) return fail(DITTO_ERR_ARG, "ditto_call_opts.class_rows must be >= -1 (-1 inherit, 0 the launch's own rows)");
    if (o->residual_bf16 < -1 || o->residual_bf16 > 1) return fail(DITTO_ERR_ARG, "ditto_call_opts.residual_bf16 must be -1, 0 or 1");
    if (o->fr_mask < -1 || o->fr_mask > 3) return fail(DITTO_ERR_ARG, "ditto_call_opts.fr_mask must be in [-1, 3]");
    if (o->lnq != -1 && o->lnq != 0 && o->lnq != 16 && o->lnq != 32) return fail(DITTO_ERR_ARG, "ditto_call_opts.lnq must be -1, 0, 16 or 32");
    for (int r : o->reserved) if (r) return fail(DITTO_ERR_ARG, "ditto_call_opts.reserved must be zero");
    return DITTO_OK;
}

}  // namespace ditto

namespace {

// roctx ranges per kernel class (DITTO_ROCTX=1): resolved once from the profiler's marker library; absent library or
// unset variable = no-ops.  The ranges are host-side brackets around the enqueue, which is what rocprofv3's marker
// trace correlates kernel dispatches with.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char* e = getenv("DITTO_ROCTX");
        if (!e || !*e || *e == '0') return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
static Roctx g_roctx;

struct ProfScope {
    ditto_model* m; hipStream_t s; int kc; hipEvent_t a = nullptr, b = nullptr;
    bool marked = false;
    ProfScope(ditto_model* m_, hipStream_t s_, int kc_) : m(m_), s(s_), kc(kc_) {
        if (g_roctx.push) { g_roctx.push(ditto_kernel_class_name(kc)); marked = true; }
        if (!m->prof) return;
        a = take(); b = take();
        if (a) (void)hipEventRecord(a, s);
    }
    hipEvent_t take() {
        if (!m->pool.empty()) { hipEvent_t e = m->pool.back(); m->pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    ~ProfScope() {
        if (marked) g_roctx.pop();
        if (!m->prof || !a || !b) return;
        (void)hipEventRecord(b, s);
        m->recs.push_back({a, b, kc});
    }
};

}  // namespace

// the workspace of one call, sliced by its plan (`h` is the caller's own buffer in ditto_block_forward); utt / pos: the row maps of a
// packed batch (launch_packed_row_map writes them at the head of every packed forward), null otherwise
struct Ws { float* h; void* u; char* qkv; void* act; char* xcat; float* eps; void* attn; size_t attn_bytes; float* splitk; size_t splitk_bytes; int32_t *utt, *pos; };
static Ws slice_ws(const WsPlan& w, void* workspace) {
    char* ws = (char*)workspace;
    return {(float*)(ws + w.h), ws + w.u, ws + w.qkv, ws + w.act, ws + w.xcat, (float*)(ws + w.eps), ws + w.attn, w.attn_bytes,
            (float*)(ws + w.splitk), w.splitk_bytes, w.pos ? (int32_t*)(ws + w.utt) : nullptr, w.pos ? (int32_t*)(ws + w.pos) : nullptr};
}

struct Rope { const float *cos, *sin; };   // the [N, head_dim / 2] tables of ditto_rope_tables
struct Buf { void* p; size_t bytes; };     // a caller-owned workspace
// what one block inherits from / hands to its neighbours in ditto_forward's chain (a lone ditto_block_forward: the defaults)
struct BlockChain {
    bool ln1_done = false;                                   // this block's norm1 output is already in u
    const float *next_g1 = nullptr, *next_be1 = nullptr;     // fc2's launch also writes the NEXT block's norm1 into u
    float *tap_self = nullptr, *tap_cross = nullptr;         // fp32 copies of h after the self- / cross-attention segment
    char* xcat = nullptr;                                    // last block: fc2 also writes bf16(h_L) into xcat's second half
};

// an _opts entry: the call's options validated, then in force on this thread for the length of f()
template <class F> static int with_opts(const ditto_call_opts* opts, F&& f) {
    if (int rc = check_call_opts(opts)) return rc;
    CallScope scope(opts);
    return f();
}

// One DiT block (reference src/components/DiT.py:100-157) on the residual stream `h`, in place; WHICH launches: `fp` (forward_plan.hip)
static int run_block(ditto_model* m, int l, const Ws& ws, const char* kv, int kv_layer, Rope rope, const BatchLayout& lay,
                     const ForwardPlan& fp, const BlockChain& ch, hipStream_t s) {
    float* const h = ws.h; void* const u = ws.u; char* const qkv = ws.qkv; void* const act = ws.act;
    const bool hb = fp.hb, fr_out = fp.fr_out, fr_fc2 = fp.fr_fc2;
    const ditto_config& c = m->cfg;
    const int d = c.hidden_dim, H = c.num_heads, dh = d / H, M = lay.M, kv_ld = c.num_layers * 2 * cfg_dp(c);
    const float scale = 1.0f / sqrtf((float)dh);
    const bool fused_rope = (dh == 64);
    // padded heads (head_dim % 64 != 0): q / k / v and the attention outputs are dp = H * dhp wide, heads at a stride of dhp
    // (zero pads: the packed weights have zero rows / columns there), the attention runs the GEMM-composed path on dhp-wide
    // heads with the TRUE head_dim's softmax scale; the self-attention's head merge + residual is a compaction pass
    const int dhp = cfg_dhp(c), dp = cfg_dp(c);
    const bool pad = dp != d;
    const bool fp8 = (c.flags & DITTO_CFG_FP8_LINEAR) != 0;   // u / act hold fp8 bytes for the fp8 GEMMs
    const LayerPack& lp = m->layers[l];
    // fr_out / fr_fc2: full-row GEMM with the residual add and the FOLLOWING LayerNorm fused (gemm_fr.hip): cross out-proj + norm3 (at
    // d = 1024 also in the fp8 configuration, with the LayerNorm output written as fp8), fc2 + the next block's norm1 (ch.ln1_done)
    // tiles per utterance: the K-loop rotation period (gemm_fr.hip).  A varlen batch runs unrotated (here and in gemm_lnq's): the
    // rotation is a function of the PADDED N, and an utterance's bits must not depend on the padding
    const bool varlen = lay.varlen();
    const int fr_rot = lay.rot_period(128);
    // variable-length batches: the attention kernels bound every utterance by its own lengths (attention_varlen.hip); every other
    // launch is row-wise and computes the padding rows too (their results never reach a valid row)
    if (varlen && (dh != 64 || pad)) {
        return fail(DITTO_ERR_SHAPE, "variable-length batches need head_dim 64 (this model's is %d)", dh);
    }
        // ---- self-attention (src/components/DiT.py:103-139) ----
        if (!ch.ln1_done) {
            ProfScope ps(m, s, DITTO_KC_LAYERNORM);
            if (fp8) HIP_TRY(launch_layernorm_fp8(h, lp.g1, lp.be1, u, d, M, d, s));
            else if (hb) HIP_TRY(launch_layernorm_xbf16(h, lp.g1, lp.be1, u, d, M, d, s));
            else HIP_TRY(launch_layernorm(h, lp.g1, lp.be1, u, d, M, d, s));
        }
        {
            ProfScope ps(m, s, DITTO_KC_GEMM_QKV);
            GemmArgs g{};
            g.A = u; g.lda = d; g.W = lp.Wqkv; g.bias = lp.bqkv; g.out = qkv; g.ldo = 3 * dp;
            g.M = M; g.N = 3 * dp; g.K = d;
            g.rope_cos = rope.cos; g.rope_sin = rope.sin; g.rope_rows_per_batch = lay.rope_rows_per_batch(); g.rope_cols = 2 * d;
            if (fused_rope && !(g_gemm_flags & 1024)) g.rope_freq_rev = m->invf_rev;   // flag 1024: A/B, table loads
            g.fp8 = fp8; g.wscale = fp8 ? lp.sqkv : nullptr;
            // packed batch: every row's position inside its utterance from the row map (the table-free angles of the same float
            // position: the padded layout's bits)
            const GemmEpilogue qkv_epi = lay.kind == BatchLayout::PACKED ? EPI_QKV_ROPE_PACKED : EPI_QKV_ROPE;
            g.rope_pos = ws.pos;
#ifdef DITTO_DIAG_QKV_PLAIN   // tools/build_diag.sh: the QKV GEMM with the plain bias epilogue (NO RoPE: wrong results) — what
                              // would the 256 x 192 kernel (whole tile rounds at M = 32768; gemm_tile 192) buy this class?
            HIP_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
#else
            if (fp.q_split) {   // "qkv_split": the last 256 columns (all v columns, plain bias epilogue) as a second launch
                GemmArgs gm = g, gt = g;
                gm.N = 3 * dp - 256;
                HIP_TRY(launch_gemm(gm, qkv_epi, s));
                gt.N = 256; gt.W = (const char*)lp.Wqkv + (size_t)gm.N * d * 2; gt.bias = lp.bqkv + gm.N;
                gt.out = qkv + (size_t)gm.N * 2; gt.rope_cols = 0; gt.rope_freq_rev = nullptr;
                HIP_TRY(launch_gemm(gt, EPI_BIAS_BF16, s));
            } else {
            HIP_TRY(launch_gemm(g, fused_rope ? qkv_epi : EPI_BIAS_BF16, s));
            if (!fused_rope) HIP_TRY(launch_rope_inplace(qkv, 3 * dp, rope.cos, rope.sin, M, lay.rope_rows_per_batch(), 2 * dp, dh, s, 1.0f, dhp));
            }
#endif
        }
        {
            ProfScope ps(m, s, DITTO_KC_ATTN_SELF);
            AttnArgs a{};
            a.q = qkv; a.ldq = 3 * dp; a.k = qkv + (size_t)dp * 2; a.ldk = 3 * dp; a.v = qkv + (size_t)2 * dp * 2;
            a.ldv = 3 * dp; a.H = H; a.dh = dhp;
            a.scale = scale; a.workspace = ws.attn; a.workspace_bytes = ws.attn_bytes; a.q_prescaled = (dh == 64);
            lay.fill_attn(a, false);
            if (pad) {   // O at the padded stride into `act` (free here), then h[:, hd dh + c] += O[:, hd dhp + c]
                a.out_bf16 = act; a.ldo = dp;
                HIP_TRY(launch_attention(a, s));
                HIP_TRY(launch_head_compact_add(act, dp, h, d, M, d, dh, dhp, s));
            } else {
                a.resid_f32 = h; a.ldr = d; a.resid_bf16 = hb;
                HIP_TRY(launch_attention(a, s));
            }
        }
        if (ch.tap_self) HIP_TRY(hipMemcpyAsync(ch.tap_self, h, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
        // ---- cross-attention (src/components/DiT.py:141-148), K/V from the per-utterance cache ----
        if (fp.lnq) {   // norm2 + q-projection in one launch (gemm_lnq.hip); else LayerNorm launch + tiled GEMM
            ProfScope ps(m, s, DITTO_KC_GEMM_QPROJ);
            HIP_TRY(launch_gemm_lnq(h, d, hb, lp.g2, lp.be2, fp.lnq == 16 ? lp.WcqP32 : lp.WcqP, lp.bcq, qkv, d, M, d, fp.lnq,
                                    lay.rot_period(64), s));
        } else {
            {
                ProfScope ps(m, s, DITTO_KC_LAYERNORM);
                if (hb) HIP_TRY(launch_layernorm_xbf16(h, lp.g2, lp.be2, u, d, M, d, s));
                else HIP_TRY(launch_layernorm(h, lp.g2, lp.be2, u, d, M, d, s));
            }
            ProfScope ps(m, s, DITTO_KC_GEMM_QPROJ);
            GemmArgs g{};
            g.A = u; g.lda = d; g.W = lp.Wcq; g.bias = lp.bcq; g.out = qkv; g.ldo = dp; g.M = M; g.N = dp; g.K = d;
            HIP_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
        }
        {
            ProfScope ps(m, s, DITTO_KC_ATTN_CROSS);
            AttnArgs a{};
            a.q = qkv; a.ldq = dp; a.k = kv + (size_t)kv_layer * 2 * dp * 2; a.ldk = kv_ld;
            a.v = kv + ((size_t)kv_layer * 2 * dp + dp) * 2; a.ldv = kv_ld; a.out_bf16 = u; a.ldo = dp;
            a.H = H; a.dh = dhp; a.scale = scale;
            a.workspace = ws.attn; a.workspace_bytes = ws.attn_bytes; a.q_prescaled = (dh == 64);
            lay.fill_attn(a, true);
            HIP_TRY(launch_attention(a, s));
        }
        bool ln3_done = false;
        if (fr_out) {
            // out-proj + residual + norm3 in one launch.  A = the attention output in u; the LayerNorm output goes to the first
            // M x d of the qkv buffer (the cross q it held has been consumed) because u is still being read as the A operand
            ProfScope ps(m, s, DITTO_KC_GEMM_OUTPROJ);
            GemmParams gp{};
            gp.A = (const bf16*)u; gp.lda = d; gp.W = (const bf16*)lp.WcoP; gp.ldw = d; gp.w_rows = d; gp.bias = lp.bco;
            gp.residual = h; gp.ldr = d; gp.out = h; gp.ldo = d; gp.M = M; gp.N = d; gp.K = d;
            HIP_TRY(launch_gemm_fr(gp, lp.g3, lp.be3, qkv, d, fr_rot, s, fp8, hb));
        } else {
            ProfScope ps(m, s, DITTO_KC_GEMM_OUTPROJ);
            GemmArgs g{};
            g.A = u; g.lda = dp; g.W = lp.Wco; g.bias = lp.bco; g.residual = h; g.ldr = d; g.out = h; g.ldo = d;
            g.M = M; g.N = d; g.K = dp;
            if (const int nso = fp.ns_out; nso > 1) {
                // low-latency class: K-splits + a finish that adds bias + residual AND writes norm3 (into qkv: u is the A operand)
                g.bias = nullptr; g.residual = nullptr; g.out = ws.splitk; g.k_splits = nso; g.split_stride = (size_t)M * d;
                HIP_TRY(launch_gemm(g, EPI_BIAS_F32, s));
                HIP_TRY(launch_splitk_finish(ws.splitk, nso, (size_t)M * d, lp.bco, h, h, nullptr, 0, M, d, s, lp.g3, lp.be3, qkv, d));
                ln3_done = true;
            } else {
                HIP_TRY(launch_gemm(g, EPI_BIAS_RES_F32, s));
            }
        }
        if (ch.tap_cross) HIP_TRY(hipMemcpyAsync(ch.tap_cross, h, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
        // ---- gated MLP (src/components/DiT.py:150-155) ----
        const void* u3 = (fr_out || ln3_done) ? (const void*)qkv : (const void*)u;   // where norm3's output is
        if (!fr_out && !ln3_done) {
            ProfScope ps(m, s, DITTO_KC_LAYERNORM);
            if (fp8) HIP_TRY(launch_layernorm_fp8(h, lp.g3, lp.be3, u, d, M, d, s));
            else HIP_TRY(launch_layernorm(h, lp.g3, lp.be3, u, d, M, d, s));
        }
        {
            ProfScope ps(m, s, DITTO_KC_GEMM_GATED);
            GemmArgs g{};
            g.A = u3; g.lda = d; g.W = lp.W1g; g.bias = lp.b1g; g.out = act; g.ldo = 4 * d; g.M = M; g.N = 8 * d;
            g.K = d; g.fp8 = fp8; g.wscale = fp8 ? lp.s1g : nullptr;
            HIP_TRY(launch_gemm(g, fp8 ? EPI_GATED_FP8 : EPI_GATED, s));
        }
        if (fr_fc2) {
            // fc2 + residual (+ the NEXT block's norm1 into u, or the bf16 copy of h_L for proj_out on the last block)
            ProfScope ps(m, s, DITTO_KC_GEMM_FC2);
            GemmParams gp{};
            gp.A = (const bf16*)act; gp.lda = 4 * d; gp.W = (const bf16*)lp.W2P; gp.ldw = 4 * d; gp.w_rows = d; gp.bias = lp.b2;
            gp.residual = h; gp.ldr = d; gp.out = h; gp.ldo = d; gp.M = M; gp.N = d; gp.K = 4 * d;
            if (ch.xcat && hb) { gp.out = ch.xcat + (size_t)d * 2; gp.ldo = 2 * d; }   // bf16 h_L IS proj_out's operand
            else if (ch.xcat) { gp.out2 = (bf16*)(ch.xcat + (size_t)d * 2); gp.ldo2 = 2 * d; }
            HIP_TRY(launch_gemm_fr(gp, ch.next_g1, ch.next_be1, ch.next_g1 ? u : nullptr, d, fr_rot, s, false, hb));
        } else {
            ProfScope ps(m, s, DITTO_KC_GEMM_FC2);
            GemmArgs g{};
            g.A = act; g.lda = 4 * d; g.W = lp.W2; g.bias = lp.b2; g.residual = h; g.ldr = d; g.out = h; g.ldo = d;
            g.M = M; g.N = d; g.K = 4 * d; g.fp8 = fp8; g.wscale = fp8 ? lp.s2 : nullptr;
            void* out2 = ch.xcat ? ch.xcat + (size_t)d * 2 : nullptr;   // bf16(h_L) for proj_out
            if (const int ns = fp.ns_fc2; ns > 1) {
                g.bias = nullptr; g.residual = nullptr; g.out = ws.splitk; g.k_splits = ns;
                g.split_stride = (size_t)M * d;
                HIP_TRY(launch_gemm(g, EPI_BIAS_F32, s));
                // (ch.next_g1 set: the finish also writes the NEXT block's norm1 into u — the plan's chain_ll)
                HIP_TRY(launch_splitk_finish(ws.splitk, ns, (size_t)M * d, lp.b2, h, h, out2, 2 * d, M, d, s, ch.next_g1, ch.next_be1,
                                             ch.next_g1 ? u : nullptr, d));
            } else {
                if (out2) { g.out2_bf16 = out2; g.ldo2 = 2 * d; }
                HIP_TRY(launch_gemm(g, EPI_BIAS_RES_F32, s));
            }
        }
    return DITTO_OK;
}

extern "C" {

int ditto_abi_version(void) { return DITTO_ABI_VERSION; }
const char* ditto_last_error(void) { return ditto::g_err; }

const char* ditto_kernel_class_name(int kc) {
    static const char* names[DITTO_KC_COUNT] = {"layernorm", "gemm_qkv_rope", "gemm_q_proj", "gemm_out_proj",
                                                "gemm_gated_mlp", "gemm_fc2", "gemm_final", "attn_self", "attn_cross",
                                                "adaln", "p_sample_update"};
    return (kc >= 0 && kc < DITTO_KC_COUNT) ? names[kc] : "?";
}

size_t ditto_arena_bytes(const ditto_config* cfg) {
    if (check_cfg(cfg) != DITTO_OK) return 0;
    return plan_arena(*cfg).total;
}
size_t ditto_cond_bytes(const ditto_config* cfg, int B, int T) {
    if (check_cfg(cfg) != DITTO_OK || B <= 0 || T <= 0) return 0;
    const size_t d = cfg->hidden_dim, dp = cfg_dp(*cfg);
    return al((size_t)B * T * cfg->num_layers * 2 * dp * 2) + al((size_t)B * 2 * d * 4);
}
size_t ditto_workspace_bytes(const ditto_config* cfg, int B, int N, int T) {
    if (check_cfg(cfg) != DITTO_OK || B <= 0 || N <= 0 || T <= 0) return 0;
    return plan_ws(*cfg, B, N, T).total;
}
size_t ditto_attention_workspace_bytes(int B, int H, int Sq, int Skv, int dh) {
    return attention_workspace_bytes(B, H, Sq, Skv, dh);
}

int ditto_model_create(const ditto_config* cfg, const ditto_weights* w, void* arena, size_t arena_bytes,
                       ditto_stream_t stream, ditto_model_t* out) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!w || !arena || !out || !w->layers) return fail(DITTO_ERR_ARG, "null argument to ditto_model_create");
    const ArenaPlan plan = plan_arena(*cfg);
    if (arena_bytes < plan.total)
        return fail(DITTO_ERR_SIZE, "arena too small: %zu < %zu", arena_bytes, plan.total);
    if ((uintptr_t)arena % 256) return fail(DITTO_ERR_ARG, "arena must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int d = cfg->hidden_dim, L = cfg->num_layers, td = cfg->time_dim, dt = cfg->text_dim;
    char* A = (char*)arena;
    std::unique_ptr<ditto_model> guard(new (std::nothrow) ditto_model());
    ditto_model* m = guard.get();
    if (!m) return fail(DITTO_ERR_ARG, "out of host memory");
    m->cfg = *cfg; m->plan = plan; m->arena = A; m->layers.resize(L);
    const int BIG = 1 << 30;
    for (int l = 0; l < L; ++l) {
        const ditto_layer_weights& lw = w->layers[l];
        const auto& q = plan.layers[l];
        const float* need[] = {lw.norm1_weight, lw.norm1_bias, lw.attn_in_proj_weight, lw.attn_in_proj_bias,
                               lw.norm2_weight, lw.norm2_bias, lw.cross_in_proj_weight, lw.cross_in_proj_bias,
                               lw.cross_out_proj_weight, lw.cross_out_proj_bias, lw.norm3_weight, lw.norm3_bias,
                               lw.mlp_fc1_weight, lw.mlp_fc1_bias, lw.gate_weight, lw.gate_bias, lw.mlp_fc2_weight,
                               lw.mlp_fc2_bias};
        for (const float* p : need)
            if (!p) return fail(DITTO_ERR_ARG, "null weight pointer in layer %d", l);
        // self-attention in_proj [3d, d] (q | k | v rows), reference src/components/DiT.py:110-114
        const bool fp8 = (cfg->flags & DITTO_CFG_FP8_LINEAR) != 0;
        // head_dim 64 (fused attention): q leaves its projection already multiplied by scale * log2(e), folded into
        // the q rows of the packed weights / biases here, so the attention kernel's scores are in log2 units
        const bool pre = (d / cfg->num_heads) == 64;
        const float qs = pre ? 1.4426950408889634f / sqrtf((float)(d / cfg->num_heads)) : 1.0f;
        const int dh_ = d / cfg->num_heads, dhp = cfg_dhp(*cfg), dp = cfg_dp(*cfg);
        const bool pad = dp != d;
        if (pad) {
            // padded heads: zero images, then every in-projection's rows / the out-projection's columns head by head
            HIP_TRY(hipMemsetAsync(A + q.Wqkv, 0, (size_t)3 * dp * d * 2, s));
            HIP_TRY(hipMemsetAsync(A + q.Wcq, 0, (size_t)dp * d * 2, s));
            HIP_TRY(hipMemsetAsync(A + q.Wco, 0, (size_t)d * dp * 2, s));
            HIP_TRY(hipMemsetAsync(A + q.bqkv, 0, (size_t)3 * dp * 4, s));
            HIP_TRY(hipMemsetAsync(A + q.bcq, 0, (size_t)dp * 4, s));
            if (l == 0) {
                HIP_TRY(hipMemsetAsync(A + plan.Wkv, 0, (size_t)L * 2 * dp * d * 2, s));
                HIP_TRY(hipMemsetAsync(A + plan.bkv, 0, (size_t)L * 2 * dp * 4, s));
            }
            for (int part = 0; part < 3; ++part) {   // q | k | v rows of attn.in_proj
                HIP_TRY(launch_pack_bf16_headrows(lw.attn_in_proj_weight + (size_t)part * d * d, A + q.Wqkv, d, d, d, dh_, dhp,
                                                  part * dp, s));
                HIP_TRY(launch_pack_vec_heads(lw.attn_in_proj_bias + part * d, (float*)(A + q.bqkv), d, dh_, dhp, part * dp, s));
            }
            HIP_TRY(launch_pack_bf16_headrows(lw.cross_in_proj_weight, A + q.Wcq, d, d, d, dh_, dhp, 0, s));
            HIP_TRY(launch_pack_vec_heads(lw.cross_in_proj_bias, (float*)(A + q.bcq), d, dh_, dhp, 0, s));
            for (int part = 0; part < 2; ++part) {   // k | v rows of cross_attn.in_proj -> the all-layer K/V projection
                HIP_TRY(launch_pack_bf16_headrows(lw.cross_in_proj_weight + (size_t)(1 + part) * d * d, A + plan.Wkv, d, d, d, dh_,
                                                  dhp, l * 2 * dp + part * dp, s));
                HIP_TRY(launch_pack_vec_heads(lw.cross_in_proj_bias + (1 + part) * d, (float*)(A + plan.bkv), d, dh_, dhp,
                                              l * 2 * dp + part * dp, s));
            }
            HIP_TRY(launch_pack_bf16_headcols(lw.cross_out_proj_weight, A + q.Wco, d, d, dp, dh_, dhp, s));
            HIP_TRY(launch_pack_bf16(lw.mlp_fc1_weight, A + q.W1g, 4 * d, d, d, 0, 16, 2, 0, s));
            HIP_TRY(launch_pack_bf16(lw.gate_weight, A + q.W1g, 4 * d, d, d, 0, 16, 2, 16, s));
            HIP_TRY(launch_pack_bf16(lw.mlp_fc2_weight, A + q.W2, d, 4 * d, 4 * d, 0, BIG, 1, 0, s));
        } else {
        if (fp8) {
            HIP_TRY(launch_pack_fp8(lw.attn_in_proj_weight, A + q.Wqkv, (float*)(A + q.sqkv), 3 * d, d, d, BIG, 1, 0, s));
            HIP_TRY(launch_pack_fp8(lw.mlp_fc1_weight, A + q.W1g, (float*)(A + q.s1g), 4 * d, d, d, 16, 2, 0, s));
            HIP_TRY(launch_pack_fp8(lw.gate_weight, A + q.W1g, (float*)(A + q.s1g), 4 * d, d, d, 16, 2, 16, s));
            HIP_TRY(launch_pack_fp8(lw.mlp_fc2_weight, A + q.W2, (float*)(A + q.s2), d, 4 * d, 4 * d, BIG, 1, 0, s));
        } else {
        HIP_TRY(launch_pack_bf16(lw.attn_in_proj_weight, A + q.Wqkv, d, d, d, 0, BIG, 1, 0, s, qs));
        HIP_TRY(launch_pack_bf16(lw.attn_in_proj_weight + (size_t)d * d, A + q.Wqkv, 2 * d, d, d, 0, BIG, 1, d, s));
        HIP_TRY(launch_pack_bf16(lw.mlp_fc1_weight, A + q.W1g, 4 * d, d, d, 0, 16, 2, 0, s));
        HIP_TRY(launch_pack_bf16(lw.gate_weight, A + q.W1g, 4 * d, d, d, 0, 16, 2, 16, s));
        HIP_TRY(launch_pack_bf16(lw.mlp_fc2_weight, A + q.W2, d, 4 * d, 4 * d, 0, BIG, 1, 0, s));
        }
        HIP_TRY(hipMemcpyAsync(A + q.bqkv, lw.attn_in_proj_bias, 3 * d * 4, hipMemcpyDeviceToDevice, s));
        // cross-attention: q rows [0,d) per layer; k,v rows [d,3d) go to the all-layer Wkv
        HIP_TRY(launch_pack_bf16(lw.cross_in_proj_weight, A + q.Wcq, d, d, d, 0, BIG, 1, 0, s, qs));
        HIP_TRY(hipMemcpyAsync(A + q.bcq, lw.cross_in_proj_bias, d * 4, hipMemcpyDeviceToDevice, s));
        if (pre) {
            HIP_TRY(launch_scale_vec((float*)(A + q.bqkv), d, qs, s));
            HIP_TRY(launch_scale_vec((float*)(A + q.bcq), d, qs, s));
            if (fp8) HIP_TRY(launch_scale_vec((float*)(A + q.sqkv), d, qs, s));   // fp8: per-row weight scale carries it
        }
        HIP_TRY(launch_pack_bf16(lw.cross_in_proj_weight + (size_t)d * d, A + plan.Wkv, 2 * d, d, d, 0, BIG, 1,
                                 l * 2 * d, s));
        HIP_TRY(hipMemcpyAsync(A + plan.bkv + (size_t)l * 2 * d * 4, lw.cross_in_proj_bias + d, 2 * d * 4,
                               hipMemcpyDeviceToDevice, s));
        HIP_TRY(launch_pack_bf16(lw.cross_out_proj_weight, A + q.Wco, d, d, d, 0, BIG, 1, 0, s));
        }   // !pad
        const StagePacks have = stage_packs(*cfg);
        if (have.o) HIP_TRY(launch_pack_bf16_stage_major(lw.cross_out_proj_weight, A + q.WcoP, d, d, s));
        if (have.fc2) HIP_TRY(launch_pack_bf16_stage_major(lw.mlp_fc2_weight, A + q.W2P, d, 4 * d, s));
        if (have.lnq) {   // from the PACKED q-projection (it carries the folded scale * log2(e))
            HIP_TRY(launch_repack_bf16_stage_major(A + q.Wcq, A + q.WcqP, d, d, s, 16));
            if (d == 768) HIP_TRY(launch_repack_bf16_stage_major(A + q.Wcq, A + q.WcqP32, d, d, s, 32));
        }
        HIP_TRY(hipMemcpyAsync(A + q.bco, lw.cross_out_proj_bias, d * 4, hipMemcpyDeviceToDevice, s));
        // gated MLP: rows interleaved [16 x fc1 | 16 x gate] so both halves of a product meet in one lane
        HIP_TRY(launch_pack_vec(lw.mlp_fc1_bias, (float*)(A + q.b1g), 4 * d, 16, 2, 0, s));
        HIP_TRY(launch_pack_vec(lw.gate_bias, (float*)(A + q.b1g), 4 * d, 16, 2, 16, s));
        HIP_TRY(hipMemcpyAsync(A + q.b2, lw.mlp_fc2_bias, d * 4, hipMemcpyDeviceToDevice, s));
        const float* lnsrc[6] = {lw.norm1_weight, lw.norm1_bias, lw.norm2_weight, lw.norm2_bias, lw.norm3_weight,
                                 lw.norm3_bias};
        const size_t lndst[6] = {q.g1, q.be1, q.g2, q.be2, q.g3, q.be3};
        for (int i = 0; i < 6; ++i)
            HIP_TRY(hipMemcpyAsync(A + lndst[i], lnsrc[i], d * 4, hipMemcpyDeviceToDevice, s));
        LayerPack& lp = m->layers[l];
        lp.Wqkv = A + q.Wqkv; lp.Wcq = A + q.Wcq; lp.Wco = A + q.Wco; lp.W1g = A + q.W1g; lp.W2 = A + q.W2;
        lp.bqkv = (const float*)(A + q.bqkv); lp.bcq = (const float*)(A + q.bcq); lp.bco = (const float*)(A + q.bco);
        lp.b1g = (const float*)(A + q.b1g); lp.b2 = (const float*)(A + q.b2);
        lp.sqkv = (const float*)(A + q.sqkv); lp.s1g = (const float*)(A + q.s1g); lp.s2 = (const float*)(A + q.s2);
        if (have.o) lp.WcoP = A + q.WcoP;
        if (have.fc2) lp.W2P = A + q.W2P;
        if (have.lnq) { lp.WcqP = A + q.WcqP; lp.WcqP32 = d == 768 ? A + q.WcqP32 : nullptr; }
        lp.g1 = (const float*)(A + q.g1); lp.be1 = (const float*)(A + q.be1); lp.g2 = (const float*)(A + q.g2);
        lp.be2 = (const float*)(A + q.be2); lp.g3 = (const float*)(A + q.g3); lp.be3 = (const float*)(A + q.be3);
    }
    const float* gneed[] = {w->t_embedding_weight, w->time_embed_0_weight, w->time_embed_0_bias,
                            w->time_embed_2_weight, w->time_embed_2_bias, w->ada_time_mlp_weight,
                            w->ada_time_mlp_bias, w->ada_text_mlp_weight, w->ada_text_mlp_bias, w->proj_in_weight,
                            w->proj_in_bias, w->proj_out_weight, w->proj_out_bias, w->rotary_inv_freq};
    int nnull = 0;
    for (const float* p : gneed) nnull += (p == nullptr);
    if (nnull == (int)(sizeof(gneed) / sizeof(gneed[0]))) {
        // standalone DiT blocks (reference src/components/DiT.py:75-157 used without a DiTTO around them)
        m->blocks_only = true;
        m->Wkv = A + plan.Wkv; m->bkv = (const float*)(A + plan.bkv);
        m->Wfin = nullptr; m->bfin = nullptr; m->ttab = nullptr; m->wx = nullptr; m->bx = nullptr; m->invf = nullptr;
        *out = guard.release();
        return DITTO_OK;
    }
    if (nnull) return fail(DITTO_ERR_ARG, "null global weight pointer (pass ALL of them, or none for a blocks-only handle)");
    // eps = x W_in^T + h_L W_out^T + (b_in + b_out): one GEMM with K = 2d (src/model/DiTTO.py:83,93-94)
    HIP_TRY(launch_pack_bf16(w->proj_in_weight, A + plan.Wfin, d, d, 2 * d, 0, BIG, 1, 0, s));
    HIP_TRY(launch_pack_bf16(w->proj_out_weight, A + plan.Wfin, d, d, 2 * d, d, BIG, 1, 0, s));
    HIP_TRY(launch_add_vec(w->proj_in_bias, w->proj_out_bias, (float*)(A + plan.bfin), d, s));
    HIP_TRY(launch_time_table(w->t_embedding_weight, w->time_embed_0_weight, w->time_embed_0_bias,
                              w->time_embed_2_weight, w->time_embed_2_bias, w->ada_time_mlp_weight,
                              w->ada_time_mlp_bias, (float*)(A + plan.ttab), cfg->diffusion_steps, td, d, s));
    HIP_TRY(hipMemcpyAsync(A + plan.wx, w->ada_text_mlp_weight, (size_t)2 * d * dt * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(A + plan.bx, w->ada_text_mlp_bias, (size_t)2 * d * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(A + plan.invf, w->rotary_inv_freq, (size_t)(d / cfg->num_heads / 2) * 4,
                           hipMemcpyDeviceToDevice, s));
    m->Wkv = A + plan.Wkv; m->bkv = (const float*)(A + plan.bkv); m->Wfin = A + plan.Wfin;
    m->bfin = (const float*)(A + plan.bfin); m->ttab = (const float*)(A + plan.ttab);
    m->wx = (const float*)(A + plan.wx); m->bx = (const float*)(A + plan.bx); m->invf = (const float*)(A + plan.invf);
    HIP_TRY(hipMemcpyAsync(A + plan.invf_rev, w->rotary_inv_freq, (size_t)(d / cfg->num_heads / 2) * 4,
                           hipMemcpyDeviceToDevice, s));
    HIP_TRY(launch_scale_vec((float*)(A + plan.invf_rev), d / cfg->num_heads / 2, 0.15915494309189535f, s));
    m->invf_rev = (const float*)(A + plan.invf_rev);
    *out = guard.release();
    return DITTO_OK;
}

int ditto_model_destroy(ditto_model_t m) {
    if (!m) return DITTO_OK;
    for (auto& r : m->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : m->pool) (void)hipEventDestroy(e);
    delete m;
    return DITTO_OK;
}

int ditto_rope_tables(ditto_model_t m, int N, float* cos_out, float* sin_out, ditto_stream_t stream) {
    if (!m || !cos_out || !sin_out || N <= 0) return fail(DITTO_ERR_ARG, "bad argument to ditto_rope_tables");
    if (m->blocks_only) return fail(DITTO_ERR_ARG, "blocks-only handle has no rotary.inv_freq");
    HIP_TRY(launch_rope_tables(m->invf, cos_out, sin_out, N, m->cfg.hidden_dim / m->cfg.num_heads / 2,
                               (hipStream_t)stream));
    return DITTO_OK;
}

// the text precompute of a padded (rows = B * T, text_len optional) or packed (cu_text given: rows = S_T, T = max_T) conditioning,
// after the entry's own checks: bf16(text) | pooled fp32 at the front of the workspace, the K/V rows of every layer (row-wise over
// the `rows` text rows), then the per-utterance text modulation
static int text_precompute(ditto_model_t m, const float* text, const int32_t* text_len, const int32_t* cu_text, int B, int T,
                           size_t rows, void* cond, size_t cond_bytes, size_t cond_need, void* workspace, size_t workspace_bytes,
                           ditto_stream_t stream) {
    const ditto_config& c = m->cfg;
    if (cond_bytes < cond_need) return fail(DITTO_ERR_SIZE, "cond buffer too small");
    const size_t need = text_scratch_bytes(c, B, rows);
    if (workspace_bytes < need) return fail(DITTO_ERR_SIZE, "workspace too small for text precompute: %zu < %zu",
                                            workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int d = c.hidden_dim, L = c.num_layers, dp = cfg_dp(c);
    char* ws = (char*)workspace;
    void* textbf = ws;
    float* pooled = (float*)(ws + al(rows * c.text_dim * 2));
    char* kv = (char*)cond;
    float* tmod = (float*)(kv + al(rows * L * 2 * dp * 2));
    HIP_TRY(launch_cast_bf16(text, textbf, rows * c.text_dim, s));
    GemmArgs g{};
    g.A = textbf; g.lda = c.text_dim; g.W = m->Wkv; g.bias = m->bkv; g.out = kv; g.ldo = L * 2 * dp;
    g.M = (int)rows; g.N = L * 2 * dp; g.K = d;
    HIP_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
    if (cu_text) HIP_TRY(launch_text_mod_packed(text, cu_text, (int)rows, T, m->wx, m->bx, pooled, tmod, B, c.text_dim, d, s));
    else if (!m->blocks_only) HIP_TRY(launch_text_mod(text, m->wx, m->bx, pooled, tmod, B, T, c.text_dim, d, s, text_len));
    return DITTO_OK;
}

static int text_precompute_padded(ditto_model_t m, const float* text, const int32_t* text_len, int B, int T, void* cond,
                                  size_t cond_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream) {
    if (!m || !text || !cond || !workspace || B <= 0 || T <= 0)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_text_precompute");
    return text_precompute(m, text, text_len, nullptr, B, T, (size_t)B * T, cond, cond_bytes, ditto_cond_bytes(&m->cfg, B, T), workspace,
                           workspace_bytes, stream);
}

int ditto_text_precompute(ditto_model_t m, const float* text, int B, int T, void* cond, size_t cond_bytes,
                          void* workspace, size_t workspace_bytes, ditto_stream_t stream) {
    return text_precompute_padded(m, text, nullptr, B, T, cond, cond_bytes, workspace, workspace_bytes, stream);
}

int ditto_text_precompute_varlen(ditto_model_t m, const float* text, const int32_t* text_len, int B, int T, void* cond,
                                 size_t cond_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream) {
    if (!text_len) return fail(DITTO_ERR_ARG, "ditto_text_precompute_varlen: null text_len");
    return text_precompute_padded(m, text, text_len, B, T, cond, cond_bytes, workspace, workspace_bytes, stream);
}

// thread-scoped options: the stack of what ditto_call_opts_push found in force (kernels.h t_opts is the top)
static thread_local CallOpts t_opt_stack[16];
static thread_local int t_opt_depth = 0;

int ditto_call_opts_push(const ditto_call_opts* opts) {
    if (int rc = check_call_opts(opts)) return rc;
    if (t_opt_depth >= 16) return fail(DITTO_ERR_ARG, "ditto_call_opts_push: more than 16 nested scopes on this thread");
    t_opt_stack[t_opt_depth++] = t_opts;
    CallScope::apply(opts);
    return DITTO_OK;
}

int ditto_call_opts_pop(void) {
    if (t_opt_depth <= 0) return fail(DITTO_ERR_ARG, "ditto_call_opts_pop without a matching push on this thread");
    t_opts = t_opt_stack[--t_opt_depth];
    return DITTO_OK;
}

int ditto_call_opts_current(ditto_call_opts* out) {
    if (!out) return fail(DITTO_ERR_ARG, "null argument to ditto_call_opts_current");
    *out = ditto_call_opts{opt_class_rows(), opt_resid_bf16(), opt_fr_mask(), opt_lnq(), {0, 0, 0, 0}};
    return DITTO_OK;
}

// what every packed entry checks on the host (the offsets themselves live on the device: documented, clamped by the kernels)
static int check_packed(const char* who, int B, int S, int max_N, int S_T, int max_T) {
    if (B <= 0 || S <= 0 || max_N <= 0 || S_T <= 0 || max_T <= 0)
        return fail(DITTO_ERR_SHAPE, "%s: B, S, max_N, S_T and max_T must be positive", who);
    if (max_N > S || max_T > S_T || B > S || B > S_T)
        return fail(DITTO_ERR_SHAPE, "%s: need max_N <= S, max_T <= S_T and at least one row per utterance (B %d, S %d, S_T %d)", who, B,
                    S, S_T);
    if (B > 65535) return fail(DITTO_ERR_SHAPE, "%s: more than 65535 utterances", who);
    return DITTO_OK;
}
static int check_packed_model(const char* who, ditto_model_t m) {
    const ditto_config& c = m->cfg;
    if (m->blocks_only) return fail(DITTO_ERR_ARG, "%s on a blocks-only handle", who);
    if (c.hidden_dim / c.num_heads != 64) return fail(DITTO_ERR_SHAPE, "%s: packed batches need head_dim 64 (this model's is %d)", who,
                                                      c.hidden_dim / c.num_heads);
    if (c.flags & DITTO_CFG_FP8_LINEAR) return fail(DITTO_ERR_SHAPE, "%s: packed batches are not supported with fp8 linear layers", who);
    return DITTO_OK;
}

// One DiTTO.forward over a batch in any layout: eps_out fp32 [lay.M, d].  `who` names the entry in the argument errors.
static int forward_impl(const char* who, ditto_model_t m, const float* x, const void* cond, const int64_t* t, Rope rope, float* eps_out,
                        Buf wsb, ditto_stream_t stream, const BatchLayout& lay) {
    const bool packed = lay.kind == BatchLayout::PACKED;
    if (!m || !x || !cond || !t || !rope.cos || !rope.sin || !eps_out || !wsb.p ||
        (packed ? !lay.cu || !lay.cu_t : lay.B <= 0 || lay.N <= 0 || lay.T <= 0))
        return fail(DITTO_ERR_ARG, "bad argument to %s", who);
    const ditto_config& c = m->cfg;
    if (packed) {
        if (int rc = check_packed_model(who, m)) return rc;
        if (int rc = check_packed(who, lay.B, lay.M, lay.N, lay.Mt, lay.T)) return rc;
    } else if (m->blocks_only) {
        return fail(DITTO_ERR_ARG, "%s on a blocks-only handle", who);
    }
    const WsPlan w = lay.plan(c);
    if (wsb.bytes < w.total) return fail(DITTO_ERR_SIZE, "workspace too small: %zu < %zu", wsb.bytes, w.total);
    if ((uintptr_t)wsb.p % 256) return fail(DITTO_ERR_ARG, "workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int d = c.hidden_dim, L = c.num_layers, M = lay.M;
    const Ws ws = slice_ws(w, wsb.p);
    const char* kv = (const char*)cond;
    const float* tmod = (const float*)(kv + lay.tmod_offset(c));
    ForwardPlan fp;   // the kernel class of every launch below, and its two class errors, before anything is enqueued
    if (int rc = plan_forward(c, M, ws.splitk_bytes, PLAN_FORWARD, &fp)) return rc;
    const bool hb = fp.hb, ln1_in_adaln = fp.ln1_in_adaln;
    {   // GlobalAdaLN (src/components/DiT.py:25-40) + bf16 copy of the raw input for proj_in
        ProfScope ps(m, s, DITTO_KC_ADALN);
        const float *g1 = ln1_in_adaln ? m->layers[0].g1 : nullptr, *be1 = ln1_in_adaln ? m->layers[0].be1 : nullptr;
        void* u1 = ln1_in_adaln ? ws.u : nullptr;
        if (packed) {   // the row maps first (utterance and RoPE position of every packed row), then the entry with the utterance map
            HIP_TRY(launch_packed_row_map(lay.cu, lay.B, M, lay.N, ws.utt, ws.pos, s));
            HIP_TRY(launch_adaln_packed(x, m->ttab, tmod, t, c.diffusion_steps, ws.utt, ws.h, ws.xcat, 2 * d, M, d, s, hb, g1, be1, u1));
        } else {
            HIP_TRY(launch_adaln(x, m->ttab, tmod, t, c.diffusion_steps, ws.h, ws.xcat, 2 * d, lay.B, lay.N, d, s, hb, g1, be1, u1));
        }
    }
    const bool chain = fp.chain_ln1 || fp.chain_ll;
    for (int l = 0; l < L; ++l) {
        BlockChain ch;
        ch.ln1_done = l > 0 ? chain : ln1_in_adaln;
        if (chain && l + 1 < L) { ch.next_g1 = m->layers[l + 1].g1; ch.next_be1 = m->layers[l + 1].be1; }
        ch.xcat = l == L - 1 ? ws.xcat : nullptr;
        if (int rc = run_block(m, l, ws, kv, l, rope, lay, fp, ch, s)) return rc;
    }
    {   // eps = proj_in(x_raw) + proj_out(h_L)  (src/model/DiTTO.py:83,93-94), one K = 2d GEMM
        ProfScope ps(m, s, DITTO_KC_GEMM_FINAL);
        GemmArgs g{};
        g.A = ws.xcat; g.lda = 2 * d; g.W = m->Wfin; g.bias = m->bfin; g.out = eps_out; g.ldo = d; g.M = M; g.N = d;
        g.K = 2 * d;
        if (const int ns = fp.ns_fin; ns > 1) {
            float* part = ws.splitk;
            g.bias = nullptr; g.out = part; g.k_splits = ns; g.split_stride = (size_t)M * d;
            HIP_TRY(launch_gemm(g, EPI_BIAS_F32, s));
            HIP_TRY(launch_splitk_finish(part, ns, (size_t)M * d, m->bfin, nullptr, eps_out, nullptr, 0, M, d, s));
        } else {
            HIP_TRY(launch_gemm(g, EPI_BIAS_F32, s));
        }
    }
    if (lay.speech_len) HIP_TRY(launch_zero_rows_past_len(eps_out, lay.speech_len, lay.B, lay.N, d, s));   // eps rows >= N_b are exactly 0
    return DITTO_OK;
}

int ditto_forward(ditto_model_t m, const float* x, const void* cond, const int64_t* t, int B, int N, int T,
                  const float* rope_cos, const float* rope_sin, float* eps_out, void* workspace,
                  size_t workspace_bytes, ditto_stream_t stream) {
    return forward_impl("ditto_forward", m, x, cond, t, {rope_cos, rope_sin}, eps_out, {workspace, workspace_bytes}, stream,
                        BatchLayout::dense(B, N, T));
}

int ditto_forward_opts(ditto_model_t m, const float* x, const void* cond, const int64_t* t, int B, int N, int T,
                       const float* rope_cos, const float* rope_sin, float* eps_out, void* workspace,
                       size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    return with_opts(opts, [&] { return ditto_forward(m, x, cond, t, B, N, T, rope_cos, rope_sin, eps_out, workspace, workspace_bytes, stream); });
}

int ditto_forward_varlen_opts(ditto_model_t m, const float* x, const void* cond, const int64_t* t, const int32_t* speech_len,
                              const int32_t* text_len, int B, int N, int T, const float* rope_cos, const float* rope_sin,
                              float* eps_out, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                              const ditto_call_opts* opts) {
    if (!speech_len || !text_len) return fail(DITTO_ERR_ARG, "ditto_forward_varlen_opts: null speech_len / text_len");
    return with_opts(opts, [&] {
        return forward_impl("ditto_forward", m, x, cond, t, {rope_cos, rope_sin}, eps_out, {workspace, workspace_bytes}, stream,
                            BatchLayout::padded(B, N, T, speech_len, text_len));
    });
}

// ---- packed batches: utterances concatenated along the rows, described by device int32 offsets [B + 1] ----
size_t ditto_packed_workspace_bytes(const ditto_config* cfg, int B, int S, int S_T) {
    if (check_cfg(cfg) != DITTO_OK || B <= 0 || S <= 0 || S_T <= 0) return 0;
    return plan_ws_packed(*cfg, B, S, S_T).total;
}
size_t ditto_packed_cond_bytes(const ditto_config* cfg, int B, int S_T) {
    if (check_cfg(cfg) != DITTO_OK || B <= 0 || S_T <= 0) return 0;
    const size_t d = cfg->hidden_dim, dp = cfg_dp(*cfg);
    return al((size_t)S_T * cfg->num_layers * 2 * dp * 2) + al((size_t)B * 2 * d * 4);
}

int ditto_text_precompute_packed(ditto_model_t m, const float* text, const int32_t* cu_text, int B, int S_T, int max_T, void* cond,
                                 size_t cond_bytes, void* workspace, size_t workspace_bytes, ditto_stream_t stream) {
    if (!m || !text || !cu_text || !cond || !workspace) return fail(DITTO_ERR_ARG, "bad argument to ditto_text_precompute_packed");
    if (int rc = check_packed_model("ditto_text_precompute_packed", m)) return rc;
    if (int rc = check_packed("ditto_text_precompute_packed", B, S_T, 1, S_T, max_T)) return rc;
    return text_precompute(m, text, nullptr, cu_text, B, max_T, (size_t)S_T, cond, cond_bytes, ditto_packed_cond_bytes(&m->cfg, B, S_T),
                           workspace, workspace_bytes, stream);
}

int ditto_forward_packed_opts(ditto_model_t m, const float* x, const void* cond, const int64_t* t, const int32_t* cu_speech,
                              const int32_t* cu_text, int B, int S, int max_N, int S_T, int max_T, const float* rope_cos,
                              const float* rope_sin, float* eps_out, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                              const ditto_call_opts* opts) {
    return with_opts(opts, [&] {
        return forward_impl("ditto_forward_packed_opts", m, x, cond, t, {rope_cos, rope_sin}, eps_out, {workspace, workspace_bytes}, stream,
                            BatchLayout::packed(B, S, max_N, S_T, max_T, cu_speech, cu_text));
    });
}

int ditto_block_forward(ditto_model_t m, int layer, float* h, const void* cond, int cond_layer, int B, int N, int T,
                        const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                        ditto_stream_t stream) {
    return ditto_block_forward_taps(m, layer, h, cond, cond_layer, B, N, T, rope_cos, rope_sin, nullptr, nullptr,
                                    workspace, workspace_bytes, stream);
}

int ditto_block_forward_taps(ditto_model_t m, int layer, float* h, const void* cond, int cond_layer, int B, int N,
                             int T, const float* rope_cos, const float* rope_sin, float* tap_self, float* tap_cross,
                             void* workspace, size_t workspace_bytes, ditto_stream_t stream) {
    if (!m || !h || !cond || !rope_cos || !rope_sin || !workspace || B <= 0 || N <= 0 || T <= 0)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_block_forward");
    const ditto_config& c = m->cfg;
    if (layer < 0 || layer >= c.num_layers || cond_layer < 0 || cond_layer >= c.num_layers)
        return fail(DITTO_ERR_ARG, "layer index out of range");
    const WsPlan w = plan_ws(c, B, N, T);
    if (workspace_bytes < w.total) return fail(DITTO_ERR_SIZE, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    Ws ws = slice_ws(w, workspace); ws.h = h;
    BlockChain ch; ch.tap_self = tap_self; ch.tap_cross = tap_cross;
    ForwardPlan fp;   // a lone block: no norm1 chain, the fp32 stream
    if (int rc = plan_forward(c, B * N, ws.splitk_bytes, PLAN_BLOCK, &fp)) return rc;
    return run_block(m, layer, ws, (const char*)cond, cond_layer, {rope_cos, rope_sin}, BatchLayout::dense(B, N, T), fp, ch, (hipStream_t)stream);
}

size_t ditto_global_adaln_scratch_bytes(int B, int d, int time_dim, int text_dim) {
    return al((size_t)B * time_dim * 4) + al((size_t)B * text_dim * 4) + 2 * al((size_t)B * 2 * d * 4);
}

int ditto_global_adaln(const float* x, const float* time_emb, const float* text_emb, const float* time_w,
                       const float* time_b, const float* text_w, const float* text_b, int B, int N, int T, int d,
                       int time_dim, int text_dim, float* out, void* scratch, size_t scratch_bytes,
                       ditto_stream_t stream) {
    if (!x || !time_emb || !text_emb || !time_w || !time_b || !text_w || !text_b || !out || !scratch || B <= 0 ||
        N <= 0 || T <= 0)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_global_adaln");
    if (d % 4 || d > 2048) return fail(DITTO_ERR_SHAPE, "d must be a multiple of 4 and <= 2048");
    if (scratch_bytes < ditto_global_adaln_scratch_bytes(B, d, time_dim, text_dim))
        return fail(DITTO_ERR_SIZE, "scratch too small for ditto_global_adaln");
    hipStream_t s = (hipStream_t)stream;
    char* sc = (char*)scratch;
    float* pooled_t = (float*)sc;                 sc += al((size_t)B * time_dim * 4);
    float* pooled_x = (float*)sc;                 sc += al((size_t)B * text_dim * 4);
    float* mod_t = (float*)sc;                    sc += al((size_t)B * 2 * d * 4);
    float* mod_x = (float*)sc;
    // time half: Linear(SiLU(time_emb)) == the text-mod kernel with a "sequence" of length 1
    HIP_TRY(launch_text_mod(time_emb, time_w, time_b, pooled_t, mod_t, B, 1, time_dim, d, s));
    HIP_TRY(launch_text_mod(text_emb, text_w, text_b, pooled_x, mod_x, B, T, text_dim, d, s));
    HIP_TRY(launch_adaln(x, mod_t, mod_x, nullptr, B, out, nullptr, 0, B, N, d, s));
    return DITTO_OK;
}

int ditto_apply_rope_f32(const float* pos, const float* t, float* out, int B, int N, int H, int dh,
                         ditto_stream_t stream) {
    if (!pos || !t || !out || B <= 0 || N <= 0 || H <= 0 || dh <= 0 || (dh & 1))
        return fail(DITTO_ERR_ARG, "bad argument to ditto_apply_rope_f32");
    if (t == out) return fail(DITTO_ERR_ARG, "ditto_apply_rope_f32 is not in-place");
    HIP_TRY(launch_apply_rope_f32(pos, t, out, B, N, H, dh, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_p_sample_update(float* x, const float* eps, const float* noise, const int64_t* t, const float* betas,
                          const float* alphas, const float* alphas_cumprod, int B, size_t elems_per_utt,
                          ditto_stream_t stream) {
    if (!x || !eps || !t || !betas || !alphas || !alphas_cumprod || B <= 0 || elems_per_utt == 0)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_p_sample_update");
    if (elems_per_utt % 4) return fail(DITTO_ERR_SHAPE, "elems_per_utt must be a multiple of 4");
    HIP_TRY(launch_p_sample_update(x, eps, noise, t, betas, alphas, alphas_cumprod, B, elems_per_utt,
                                   (hipStream_t)stream));
    return DITTO_OK;
}

// what every step entry does after its own checks: the workspace against the layout's plan, then the forward into the plan's eps
// slot (returned in *eps); the entry's own update launch follows
static int step_forward(const char* who, ditto_model_t m, const float* x, const void* cond, const int64_t* t, Rope rope, Buf wsb,
                        ditto_stream_t stream, const BatchLayout& lay, float** eps) {
    const WsPlan w = lay.plan(m->cfg);
    if (wsb.bytes < w.total) return fail(DITTO_ERR_SIZE, "workspace too small: %zu < %zu", wsb.bytes, w.total);
    *eps = (float*)((char*)wsb.p + w.eps);
    return forward_impl(who, m, x, cond, t, rope, *eps, wsb, stream, lay);
}

// one reverse-diffusion step after the entry's own checks: the forward, then the update with z from `noise` or, with seeds, from
// Philox of (seed, step); varlen (lay.speech_len given): rows past each length of x then become 0.  The noise of element i of an
// utterance is a function of (seed, step, i): in the padded layout i is the same row-major index as at the utterance's own length, so
// a varlen trajectory is comparable to the solo one.
static int p_sample_step(ditto_model_t m, float* x, const void* cond, const int64_t* t, const float* noise, const int64_t* seeds,
                         uint32_t step, const float* betas, const float* alphas, const float* alphas_cumprod, Rope rope, Buf wsb,
                         ditto_stream_t stream, const BatchLayout& lay) {
    float* eps;
    if (int rc = step_forward("ditto_forward", m, x, cond, t, rope, wsb, stream, lay, &eps)) return rc;
    ProfScope ps(m, (hipStream_t)stream, DITTO_KC_UPDATE);
    const int B = lay.B, N = lay.N;
    const size_t per = (size_t)N * m->cfg.hidden_dim;   // a multiple of 64 (check_cfg): what the update kernels' float4 rows need
    if (seeds) HIP_TRY(launch_p_sample_update_seeded(x, eps, seeds, step, t, betas, alphas, alphas_cumprod, B, per, (hipStream_t)stream));
    else if (int rc = ditto_p_sample_update(x, eps, noise, t, betas, alphas, alphas_cumprod, B, per, stream)) return rc;
    if (lay.speech_len) HIP_TRY(launch_zero_rows_past_len(x, lay.speech_len, B, N, m->cfg.hidden_dim, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_p_sample(ditto_model_t m, float* x, const void* cond, const int64_t* t, const float* noise,
                   const float* betas, const float* alphas, const float* alphas_cumprod, int B, int N, int T,
                   const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                   ditto_stream_t stream) {
    if (!m || !workspace) return fail(DITTO_ERR_ARG, "bad argument to ditto_p_sample");
    return p_sample_step(m, x, cond, t, noise, nullptr, 0, betas, alphas, alphas_cumprod, {rope_cos, rope_sin}, {workspace, workspace_bytes},
                         stream, BatchLayout::dense(B, N, T));
}

int ditto_p_sample_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const float* noise,
                        const float* betas, const float* alphas, const float* alphas_cumprod, int B, int N, int T,
                        const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                        ditto_stream_t stream, const ditto_call_opts* opts) {
    return with_opts(opts, [&] { return ditto_p_sample(m, x, cond, t, noise, betas, alphas, alphas_cumprod, B, N, T, rope_cos, rope_sin, workspace,
                                                       workspace_bytes, stream); });
}

int ditto_noise_normal(float* out, const int64_t* seeds, uint32_t step, int B, size_t elems_per_utt,
                       ditto_stream_t stream) {
    if (!out || !seeds || B <= 0 || elems_per_utt == 0) return fail(DITTO_ERR_ARG, "bad argument to ditto_noise_normal");
    if (elems_per_utt % 4) return fail(DITTO_ERR_SHAPE, "elems_per_utt must be a multiple of 4");
    HIP_TRY(launch_noise_normal(out, seeds, step, B, elems_per_utt, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_p_sample_seeded(ditto_model_t m, float* x, const void* cond, const int64_t* t, const int64_t* seeds,
                          uint32_t step, const float* betas, const float* alphas, const float* alphas_cumprod, int B,
                          int N, int T, const float* rope_cos, const float* rope_sin, void* workspace,
                          size_t workspace_bytes, ditto_stream_t stream) {
    if (!m || !workspace || !seeds || !betas || !alphas || !alphas_cumprod)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_p_sample_seeded");
    return p_sample_step(m, x, cond, t, nullptr, seeds, step, betas, alphas, alphas_cumprod, {rope_cos, rope_sin}, {workspace, workspace_bytes},
                         stream, BatchLayout::dense(B, N, T));
}

int ditto_p_sample_seeded_varlen_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const int64_t* seeds,
                                      const int32_t* speech_len, const int32_t* text_len, uint32_t step, const float* betas,
                                      const float* alphas, const float* alphas_cumprod, int B, int N, int T, const float* rope_cos,
                                      const float* rope_sin, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                                      const ditto_call_opts* opts) {
    if (!m || !workspace || !seeds || !betas || !alphas || !alphas_cumprod || !speech_len || !text_len)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_p_sample_seeded_varlen_opts");
    if (B <= 0 || N <= 0 || T <= 0) return fail(DITTO_ERR_SHAPE, "ditto_p_sample_seeded_varlen_opts: B, N and T must be positive");
    return with_opts(opts, [&] {
        return p_sample_step(m, x, cond, t, nullptr, seeds, step, betas, alphas, alphas_cumprod, {rope_cos, rope_sin},
                             {workspace, workspace_bytes}, stream, BatchLayout::padded(B, N, T, speech_len, text_len));
    });
}

int ditto_p_sample_varlen_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const float* noise,
                               const int32_t* speech_len, const int32_t* text_len, const float* betas, const float* alphas,
                               const float* alphas_cumprod, int B, int N, int T, const float* rope_cos, const float* rope_sin,
                               void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    if (!m || !workspace || !betas || !alphas || !alphas_cumprod || !speech_len || !text_len)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_p_sample_varlen_opts");
    if (B <= 0 || N <= 0 || T <= 0) return fail(DITTO_ERR_SHAPE, "ditto_p_sample_varlen_opts: B, N and T must be positive");
    return with_opts(opts, [&] {
        return p_sample_step(m, x, cond, t, noise, nullptr, 0, betas, alphas, alphas_cumprod, {rope_cos, rope_sin},
                             {workspace, workspace_bytes}, stream, BatchLayout::padded(B, N, T, speech_len, text_len));
    });
}

int ditto_p_sample_seeded_opts(ditto_model_t m, float* x, const void* cond, const int64_t* t, const int64_t* seeds,
                               uint32_t step, const float* betas, const float* alphas, const float* alphas_cumprod, int B,
                               int N, int T, const float* rope_cos, const float* rope_sin, void* workspace,
                               size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    return with_opts(opts, [&] { return ditto_p_sample_seeded(m, x, cond, t, seeds, step, betas, alphas, alphas_cumprod, B, N, T, rope_cos, rope_sin,
                                                              workspace, workspace_bytes, stream); });
}

int ditto_denoise_steps_opts(ditto_model_t m, float* x, const void* cond, int t_begin, int t_end, const float* noise,
                             const float* betas, const float* alphas, const float* alphas_cumprod, int B, int N, int T,
                             const float* rope_cos, const float* rope_sin, int64_t* t_scratch, void* workspace,
                             size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    return with_opts(opts, [&] { return ditto_denoise_steps(m, x, cond, t_begin, t_end, noise, betas, alphas, alphas_cumprod, B, N, T, rope_cos,
                                                            rope_sin, t_scratch, workspace, workspace_bytes, stream); });
}

int ditto_denoise_steps(ditto_model_t m, float* x, const void* cond, int t_begin, int t_end, const float* noise,
                        const float* betas, const float* alphas, const float* alphas_cumprod, int B, int N, int T,
                        const float* rope_cos, const float* rope_sin, int64_t* t_scratch, void* workspace,
                        size_t workspace_bytes, ditto_stream_t stream) {
    if (!m || !x || !t_scratch) return fail(DITTO_ERR_ARG, "bad argument to ditto_denoise_steps");
    if (t_end < 0 || t_begin < t_end || t_begin >= m->cfg.diffusion_steps)
        return fail(DITTO_ERR_ARG, "need 0 <= t_end <= t_begin < diffusion_steps");
    if (!noise && t_begin > 0) return fail(DITTO_ERR_ARG, "noise may be NULL only for the single step t = 0");
    const size_t per_step = (size_t)B * N * m->cfg.hidden_dim;
    for (int tv = t_begin, i = 0; tv >= t_end; --tv, ++i) {
        HIP_TRY(launch_fill_i64(t_scratch, B, tv, (hipStream_t)stream));
        if (int rc = ditto_p_sample(m, x, cond, t_scratch, noise ? noise + (size_t)i * per_step : nullptr, betas, alphas,
                                    alphas_cumprod, B, N, T, rope_cos, rope_sin, workspace, workspace_bytes, stream))
            return rc;
    }
    return DITTO_OK;
}

int ditto_q_sample(const float* x_start, const float* noise, const int64_t* t, const float* buffer, float* out, int B,
                   size_t elems_per_utt, ditto_stream_t stream) {
    if (!x_start || !noise || !t || !buffer || !out || B <= 0) return fail(DITTO_ERR_ARG, "bad argument to ditto_q_sample");
    if (elems_per_utt % 4) return fail(DITTO_ERR_SHAPE, "elems_per_utt must be a multiple of 4");
    HIP_TRY(launch_q_sample(x_start, noise, t, buffer, out, B, elems_per_utt, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_layernorm_bf16(const float* x, const float* gamma, const float* beta, void* out_bf16, int M, int d,
                         ditto_stream_t stream) {
    if (!x || !out_bf16 || M <= 0 || d <= 0 || (gamma == nullptr) != (beta == nullptr))
        return fail(DITTO_ERR_ARG, "bad argument to ditto_layernorm_bf16");
    if (d % 4 || d > 2048) return fail(DITTO_ERR_SHAPE, "d must be a multiple of 4 and <= 2048");
    HIP_TRY(launch_layernorm(x, gamma, beta, out_bf16, d, M, d, (hipStream_t)stream));
    return DITTO_OK;
}

// ---- the forward row kernels on their own (unit tests): one launch_* each, after the checks that keep the launch inside what the
// caller described
static bool misaligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) != 0; }

static int check_adaln_rows(const char* who, const float* x, const float* ttab, const float* tmod, int steps, const void* h_out,
                            int h_is_bf16, const void* raw_bf16, int ldraw, const float* g1, const float* be1, const void* u1_bf16,
                            long long rows, int d) {
    if (!x || !ttab || !tmod || !h_out) return fail(DITTO_ERR_ARG, "null pointer to %s", who);
    if (u1_bf16 && (!g1 || !be1)) return fail(DITTO_ERR_ARG, "%s: u1_bf16 needs g1 and be1", who);
    if (rows <= 0 || rows > 0x7FFFFFFF || d <= 0) return fail(DITTO_ERR_SHAPE, "%s: the row count and d must be positive", who);
    if (d % 4 || d > 2048) return fail(DITTO_ERR_SHAPE, "%s: d must be a multiple of 4 and <= 2048", who);
    if (steps <= 0) return fail(DITTO_ERR_SHAPE, "%s: steps (the rows of ttab) must be positive", who);
    if (raw_bf16 && (ldraw < d || ldraw % 4)) return fail(DITTO_ERR_SHAPE, "%s: ldraw must cover d columns in multiples of 4", who);
    if (misaligned(x, 16) || misaligned(ttab, 16) || misaligned(tmod, 16) || misaligned(h_out, h_is_bf16 ? 8 : 16) ||
        misaligned(raw_bf16, 8) || misaligned(g1, 16) || misaligned(be1, 16) || misaligned(u1_bf16, 8))
        return fail(DITTO_ERR_ARG, "%s: fp32 rows must be 16-byte aligned, bf16 rows 8-byte aligned", who);
    return DITTO_OK;
}

int ditto_adaln_rows(const float* x, const float* ttab, const float* tmod, const int64_t* t, int steps, void* h_out,
                     int h_is_bf16, void* raw_bf16, int ldraw, const float* g1, const float* be1, void* u1_bf16, int B, int N,
                     int d, ditto_stream_t stream) {
    const char* who = "ditto_adaln_rows";
    if (B <= 0 || N <= 0) return fail(DITTO_ERR_SHAPE, "%s: B and N must be positive", who);
    if (int rc = check_adaln_rows(who, x, ttab, tmod, steps, h_out, h_is_bf16, raw_bf16, ldraw, g1, be1, u1_bf16, (long long)B * N, d))
        return rc;
    HIP_TRY(launch_adaln(x, ttab, tmod, t, steps, (float*)h_out, raw_bf16, ldraw, B, N, d, (hipStream_t)stream, h_is_bf16 != 0,
                         u1_bf16 ? g1 : nullptr, u1_bf16 ? be1 : nullptr, u1_bf16));
    return DITTO_OK;
}

int ditto_adaln_rows_packed(const float* x, const float* ttab, const float* tmod, const int64_t* t, int steps,
                            const int32_t* utt, void* h_out, int h_is_bf16, void* raw_bf16, int ldraw, const float* g1,
                            const float* be1, void* u1_bf16, int S, int d, ditto_stream_t stream) {
    const char* who = "ditto_adaln_rows_packed";
    if (!utt) return fail(DITTO_ERR_ARG, "%s: null utt", who);
    if (int rc = check_adaln_rows(who, x, ttab, tmod, steps, h_out, h_is_bf16, raw_bf16, ldraw, g1, be1, u1_bf16, S, d)) return rc;
    HIP_TRY(launch_adaln_packed(x, ttab, tmod, t, steps, utt, (float*)h_out, raw_bf16, ldraw, S, d, (hipStream_t)stream,
                                h_is_bf16 != 0, u1_bf16 ? g1 : nullptr, u1_bf16 ? be1 : nullptr, u1_bf16));
    return DITTO_OK;
}

int ditto_splitk_finish(const float* partial, int nsplit, size_t stride, const float* bias, const float* residual, float* out,
                        void* out2_bf16, int ldo2, const float* gamma, const float* beta, void* u_bf16, int ldu, int M, int N,
                        ditto_stream_t stream) {
    const char* who = "ditto_splitk_finish";
    if (!partial || !out) return fail(DITTO_ERR_ARG, "null pointer to %s", who);
    if (u_bf16 && (!gamma || !beta)) return fail(DITTO_ERR_ARG, "%s: u_bf16 needs gamma and beta", who);
    if (nsplit <= 0 || M <= 0 || N <= 0) return fail(DITTO_ERR_SHAPE, "%s: nsplit, M and N must be positive", who);
    if (N % 4) return fail(DITTO_ERR_SHAPE, "%s: N must be a multiple of 4", who);
    if (nsplit > 1 && (stride < (size_t)M * N || stride % 4))
        return fail(DITTO_ERR_SHAPE, "%s: stride must cover M * N elements in multiples of 4", who);
    if (out2_bf16 && (ldo2 < N || ldo2 % 4)) return fail(DITTO_ERR_SHAPE, "%s: ldo2 must cover N columns in multiples of 4", who);
    if (u_bf16 && N > 2048) return fail(DITTO_ERR_SHAPE, "%s: the fused LayerNorm needs N <= 2048", who);
    if (u_bf16 && (ldu < N || ldu % 4)) return fail(DITTO_ERR_SHAPE, "%s: ldu must cover N columns in multiples of 4", who);
    if (misaligned(partial, 16) || misaligned(bias, 16) || misaligned(residual, 16) || misaligned(out, 16) ||
        misaligned(out2_bf16, 8) || misaligned(gamma, 16) || misaligned(beta, 16) || misaligned(u_bf16, 8))
        return fail(DITTO_ERR_ARG, "%s: fp32 rows must be 16-byte aligned, bf16 rows 8-byte aligned", who);
    HIP_TRY(launch_splitk_finish(partial, nsplit, stride, bias, residual, out, out2_bf16, ldo2, M, N, (hipStream_t)stream,
                                 u_bf16 ? gamma : nullptr, u_bf16 ? beta : nullptr, u_bf16, ldu));
    return DITTO_OK;
}

int ditto_text_mod(const float* text, const int32_t* text_len, const float* wx, const float* bx, float* pooled, float* tmod,
                   int B, int T, int dt, int d, ditto_stream_t stream) {
    if (!text || !wx || !bx || !pooled || !tmod) return fail(DITTO_ERR_ARG, "null pointer to ditto_text_mod");
    if (B <= 0 || T <= 0 || dt <= 0 || d <= 0 || B > 65535) return fail(DITTO_ERR_SHAPE, "ditto_text_mod: B (<= 65535), T, dt and d must be positive");
    HIP_TRY(launch_text_mod(text, wx, bx, pooled, tmod, B, T, dt, d, (hipStream_t)stream, text_len));
    return DITTO_OK;
}

int ditto_text_mod_packed(const float* text, const int32_t* cu_text, int S_T, int max_T, const float* wx, const float* bx,
                          float* pooled, float* tmod, int B, int dt, int d, ditto_stream_t stream) {
    if (!text || !cu_text || !wx || !bx || !pooled || !tmod) return fail(DITTO_ERR_ARG, "null pointer to ditto_text_mod_packed");
    if (B <= 0 || S_T <= 0 || max_T <= 0 || dt <= 0 || d <= 0 || B > 65535)
        return fail(DITTO_ERR_SHAPE, "ditto_text_mod_packed: B (<= 65535), S_T, max_T, dt and d must be positive");
    HIP_TRY(launch_text_mod_packed(text, cu_text, S_T, max_T, wx, bx, pooled, tmod, B, dt, d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_time_table(const float* emb, const float* w0, const float* b0, const float* w2, const float* b2, const float* wt,
                     const float* bt, float* ttab, int steps, int td, int d, ditto_stream_t stream) {
    if (!emb || !w0 || !b0 || !w2 || !b2 || !wt || !bt || !ttab) return fail(DITTO_ERR_ARG, "null pointer to ditto_time_table");
    if (steps <= 0 || td <= 0 || d <= 0) return fail(DITTO_ERR_SHAPE, "ditto_time_table: steps, td and d must be positive");
    if (td > 4096) return fail(DITTO_ERR_SHAPE, "ditto_time_table: td must be <= 4096 (three td-vectors are staged in the LDS)");
    HIP_TRY(launch_time_table(emb, w0, b0, w2, b2, wt, bt, ttab, steps, td, d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_packed_row_map(const int32_t* cu, int B, int S, int max_len, int32_t* utt, int32_t* pos, ditto_stream_t stream) {
    if (!cu || !utt || !pos) return fail(DITTO_ERR_ARG, "null pointer to ditto_packed_row_map");
    if (B <= 0 || S <= 0 || max_len <= 0) return fail(DITTO_ERR_SHAPE, "ditto_packed_row_map: B, S and max_len must be positive");
    HIP_TRY(launch_packed_row_map(cu, B, S, max_len, utt, pos, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_gemm_bf16(const void* A, int lda, const void* W, const float* bias, const float* residual, void* out,
                    int ldo, int M, int N, int K, int epilogue, ditto_stream_t stream) {
    if (!A || !W || !out) return fail(DITTO_ERR_ARG, "null pointer to ditto_gemm_bf16");
    if (K % 64 || N % 16 || lda % 8) return fail(DITTO_ERR_SHAPE, "need K %% 64 == 0, N %% 16 == 0, lda %% 8 == 0");
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.bias = bias; g.residual = residual; g.ldr = ldo; g.out = out; g.ldo = ldo;
    g.M = M; g.N = N; g.K = K;
    GemmEpilogue e;
    switch (epilogue) {
        case 0: e = EPI_BIAS_BF16; break;
        case 1: e = EPI_BIAS_RES_F32; break;
        case 3:
            if (!bias || N % 32) return fail(DITTO_ERR_ARG, "gated epilogue needs a bias and N %% 32 == 0");
            e = EPI_GATED; break;
        case 4: e = EPI_BIAS_F32; break;
        case 6: e = EPI_BIAS_RELU_BF16; break;
        default: return fail(DITTO_ERR_ARG, "epilogue must be 0, 1, 3, 4 or 6");
    }
    HIP_TRY(launch_gemm(g, e, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_gemm_epilogue_bf16(const ditto_gemm_epilogue_args* a, int epilogue, int* structure_out, ditto_stream_t stream) {
    const char* who = "ditto_gemm_epilogue_bf16";
    if (structure_out) *structure_out = 0;
    if (!a || !a->A || !a->W || !a->out) return fail(DITTO_ERR_ARG, "null pointer to %s", who);
    if (epilogue == 5) return fail(DITTO_ERR_ARG, "%s: epilogue 5 (fp8 output) belongs to ditto_gemm_fp8", who);
    if (epilogue < 0 || epilogue > 9) return fail(DITTO_ERR_ARG, "%s: epilogue must be 0 .. 9 (not 5)", who);
    const int M = a->M, N = a->N, K = a->K;
    if (M <= 0 || N <= 0 || K <= 0) return fail(DITTO_ERR_SHAPE, "%s: M, N and K must be positive", who);
    if (K % 64 || N % 16) return fail(DITTO_ERR_SHAPE, "%s: need K %% 64 == 0 and N %% 16 == 0", who);
    if (a->lda % 8 || a->lda < K || a->ldw % 8 || (a->ldw && a->ldw < K))
        return fail(DITTO_ERR_SHAPE, "%s: lda / ldw must cover K columns in multiples of 8 (ldw 0 = K)", who);
    if (a->w_rows < 0 || a->w_rows > N) return fail(DITTO_ERR_SHAPE, "%s: w_rows must be in [0, N] (0 = N)", who);
    const GemmEpilogue e = (GemmEpilogue)epilogue;
    const bool f32_out = e == EPI_BIAS_RES_F32 || e == EPI_BIAS_F32;
    const int out_cols = (e == EPI_GATED || e == EPI_GATED_PRE) ? N / 2 : (e == EPI_GATED_BWD ? 2 * N : N);
    if (a->ldo < out_cols || a->ldo % (f32_out ? 4 : 8))   // rows are written in 16-byte pieces
        return fail(DITTO_ERR_SHAPE, "%s: ldo must cover %d columns in multiples of %d", who, out_cols, f32_out ? 4 : 8);
    switch (e) {
        case EPI_BIAS_RES_F32:
            if (a->residual && (a->ldr < N || a->ldr % 4)) return fail(DITTO_ERR_SHAPE, "%s: ldr must cover N columns in multiples of 4", who);
            if (a->out2_bf16 && (a->ldo2 < N || a->ldo2 % 4)) return fail(DITTO_ERR_SHAPE, "%s: ldo2 must cover N columns in multiples of 4", who);
            break;
        case EPI_QKV_ROPE:
        case EPI_QKV_ROPE_PACKED:
            if (!a->rope_cos || !a->rope_sin) return fail(DITTO_ERR_ARG, "%s: the RoPE epilogues need rope_cos and rope_sin (read unless rope_freq_rev is given)", who);
            if (e == EPI_QKV_ROPE_PACKED && !a->rope_pos) return fail(DITTO_ERR_ARG, "%s: epilogue 9 needs rope_pos", who);
            if (N % 64 || a->rope_cols % 64 || a->rope_cols < 0 || a->rope_cols > N)
                return fail(DITTO_ERR_SHAPE, "%s: the RoPE epilogues need N %% 64 == 0 and 0 <= rope_cols <= N in multiples of 64", who);
            if (e == EPI_QKV_ROPE && a->rope_rows_per_batch <= 0) return fail(DITTO_ERR_SHAPE, "%s: epilogue 2 needs rope_rows_per_batch > 0", who);
            break;
        case EPI_GATED:
            if (!a->bias) return fail(DITTO_ERR_ARG, "%s: the gated epilogue needs a bias", who);
            if (N % 32) return fail(DITTO_ERR_SHAPE, "%s: the gated epilogue needs N %% 32 == 0", who);
            break;
        case EPI_GATED_PRE:
            if (!a->bias || !a->out2_bf16) return fail(DITTO_ERR_ARG, "%s: epilogue 8 needs a bias and out2_bf16", who);
            if (N % 256) return fail(DITTO_ERR_SHAPE, "%s: epilogue 8 runs on 256 x 256 tiles only: N %% 256 == 0", who);
            if (a->ldo2 < N || a->ldo2 % 8) return fail(DITTO_ERR_SHAPE, "%s: ldo2 must cover N columns in multiples of 8", who);
            break;
        case EPI_GATED_BWD:
            if (a->bias || !a->pre_bf16 || !a->colsum_partial) return fail(DITTO_ERR_ARG, "%s: epilogue 7 takes no bias and needs pre_bf16 and colsum_partial", who);
            if (N % 256 || !gemm_gated_bwd_fused_ok(M, N))
                return fail(DITTO_ERR_SHAPE, "%s: epilogue 7 needs N %% 256 == 0, N >= 2048, at least 144 tiles of 256 x 256 and gemm_tile 0 or 256", who);
            if (a->ldpre < 2 * N || a->ldpre % 8) return fail(DITTO_ERR_SHAPE, "%s: ldpre must cover 2 N columns in multiples of 8", who);
            break;
        default: break;
    }
    GemmArgs g{};
    g.A = a->A; g.lda = a->lda; g.W = a->W; g.ldw = a->ldw; g.w_rows = a->w_rows; g.bias = a->bias;
    g.residual = a->residual; g.ldr = a->ldr; g.out = a->out; g.ldo = a->ldo; g.out2_bf16 = a->out2_bf16; g.ldo2 = a->ldo2;
    g.rope_cos = a->rope_cos; g.rope_sin = a->rope_sin; g.rope_rows_per_batch = a->rope_rows_per_batch; g.rope_cols = a->rope_cols;
    g.rope_freq_rev = a->rope_freq_rev; g.rope_pos = a->rope_pos;
    g.pre_bf16 = a->pre_bf16; g.ldpre = a->ldpre; g.colsum_partial = a->colsum_partial;
    g.M = M; g.N = N; g.K = K;
    const hipError_t err = launch_gemm(g, e, (hipStream_t)stream);
    if (structure_out) *structure_out = t_gemm_structure;
    HIP_TRY(err);
    return DITTO_OK;
}

int ditto_gemm_tn_bf16(const void* X, int ldx, const void* Y, int ldy, float* out, int ldo, int Mo, int No, int K,
                       int k_splits, int tile, void* workspace, size_t workspace_bytes, ditto_stream_t stream) {
    if (!X || !Y || !out || !workspace || Mo < 8 || No < 8 || K <= 0 || (Mo | No | ldx | ldy) % 8 || ldo < No)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_gemm_tn_bf16");
    if (ldx < Mo || ldy < No) return fail(DITTO_ERR_ARG, "ditto_gemm_tn_bf16: ldx must cover Mo columns and ldy No columns");
    // the LDS-DMA moves 16 B per lane (ld % 8 keeps every row aligned once the base is); the split-K reduce stores f32x4
    if (((uintptr_t)X | (uintptr_t)Y) % 16) return fail(DITTO_ERR_ARG, "ditto_gemm_tn_bf16: X and Y must be 16-byte aligned");
    if (k_splits > 1 && (uintptr_t)out % 16) return fail(DITTO_ERR_ARG, "ditto_gemm_tn_bf16: split-K needs a 16-byte aligned out");
    if (tile != 128 && tile != 256) return fail(DITTO_ERR_ARG, "tile must be 128 or 256");
    if ((uintptr_t)workspace % 256) return fail(DITTO_ERR_ARG, "workspace must be 256-byte aligned");
    const int S = k_splits > 1 ? k_splits : 1;
    const size_t need = 256 + (S > 1 ? (size_t)S * Mo * No * 4 : 0);
    if (workspace_bytes < need) return fail(DITTO_ERR_SIZE, "workspace too small: %zu < %zu", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(workspace, 0, 256, s));
    if (S > 1) {
        if (ldo != No) return fail(DITTO_ERR_ARG, "split-K needs a contiguous output (ldo == No)");
        float* part = (float*)((char*)workspace + 256);
        HIP_TRY(launch_gemm_tn(X, ldx, Y, ldy, workspace, part, No, Mo, No, K, S, (size_t)Mo * No, s, tile == 256));
        HIP_TRY(launch_reduce_partials(part, S, (size_t)Mo * No, out, s));
    } else {
        HIP_TRY(launch_gemm_tn(X, ldx, Y, ldy, workspace, out, ldo, Mo, No, K, 1, 0, s, tile == 256));
    }
    return DITTO_OK;
}

int ditto_gemm_lnq_bf16(const void* h, int ldh, int h_is_bf16, const float* gamma, const float* beta, const void* W,
                        const float* bias, void* out_bf16, int ldo, int M, int d, int mfma_shape, void* w_scratch,
                        ditto_stream_t stream) {
    if (d != 768 && d != 1024) return fail(DITTO_ERR_SHAPE, "ditto_gemm_lnq_bf16: d must be 768 or 1024");
    if (!h || !gamma || !beta || !W || !out_bf16 || !w_scratch || M <= 0 || ldh < d || ldo < d || ldh % 4 || ldo % 8)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_gemm_lnq_bf16");
    if (mfma_shape != 32 && mfma_shape != 16) return fail(DITTO_ERR_ARG, "mfma_shape must be 32 (32x32x16) or 16 (16x16x32)");
    if (d == 1024 && (mfma_shape != 32 || h_is_bf16)) return fail(DITTO_ERR_SHAPE, "d = 1024: 32x32x16 and fp32 rows only");
    if ((uintptr_t)w_scratch % 256) return fail(DITTO_ERR_ARG, "w_scratch must be 256-byte aligned");
    // a lane loads four columns of a row at once (16 bytes of fp32, 8 of bf16; ldh % 4 keeps every row aligned once the base is) and
    // 16 bytes of gamma / beta, the bias row goes to the LDS in 16-byte pieces, and the output leaves in 16-byte stores
    if ((uintptr_t)h % (h_is_bf16 ? 8 : 16) || ((uintptr_t)out_bf16 | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)bias) % 16)
        return fail(DITTO_ERR_ARG, "ditto_gemm_lnq_bf16: h (fp32; 8 bytes for bf16), out, gamma, beta and bias must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_repack_bf16_stage_major(W, w_scratch, d, d, s, mfma_shape == 32 ? 16 : 32));
    HIP_TRY(launch_gemm_lnq(h, ldh, h_is_bf16 != 0, gamma, beta, w_scratch, bias, out_bf16, ldo, M, d, mfma_shape,
                            g_fr_rot > 1 ? g_fr_rot : 0, s));   // "fr_rot" > 1: the unit entry rotates too, with that period in tiles
    return DITTO_OK;
}

int ditto_gemm_ln_bf16(const void* A, int lda, const void* W, const float* bias, const float* residual, float* out,
                       int ldo, const float* gamma, const float* beta, void* u_bf16, int ldu, int M, int N, int K,
                       ditto_stream_t stream) {
    if (!A || !W || !out || (gamma == nullptr) != (beta == nullptr) || (gamma == nullptr) != (u_bf16 == nullptr))
        return fail(DITTO_ERR_ARG, "bad argument to ditto_gemm_ln_bf16");
    const bool ok = N == 1024 ? gemm_fr64_supports(M, N, K, (size_t)lda, (size_t)K) : gemm_fr_supports(M, N, K, (size_t)lda, (size_t)K);
    if (!ok || lda % 8 || lda < K)
        return fail(DITTO_ERR_SHAPE, "ditto_gemm_ln_bf16 needs N == 768 or N == 1024, M >= 64, K %% 64 == 0, K >= 64, lda %% 8 == 0, lda >= K");
    // Rows leave in 16-byte stores and the fp32 residual arrives in 16-byte loads (ldr = ldo): four fp32 / eight bf16 / sixteen fp8
    // elements.  A, the bias and gamma | beta go to the LDS in 16-byte pieces, the weight fragments to registers in 16-byte loads.
    const int ho = g_fr_hb ? 8 : 4, uo = g_fr_u_fp8 ? 16 : 8;
    if (ldo < N || ldo % ho) return fail(DITTO_ERR_SHAPE, "ditto_gemm_ln_bf16: ldo must cover N columns in multiples of %d", ho);
    if (u_bf16 && (ldu < N || ldu % uo)) return fail(DITTO_ERR_SHAPE, "ditto_gemm_ln_bf16: ldu must cover N columns in multiples of %d", uo);
    if (((uintptr_t)A | (uintptr_t)W | (uintptr_t)out | (uintptr_t)residual | (uintptr_t)u_bf16 | (uintptr_t)bias | (uintptr_t)gamma |
         (uintptr_t)beta) % 16)
        return fail(DITTO_ERR_ARG, "ditto_gemm_ln_bf16: A, W, out, residual, u, bias, gamma and beta must be 16-byte aligned");
    // the bf16 residual tile is fetched at 32-bit byte offsets from the residual pointer (csrc/gemm_frd.hip issue_unit)
    if (g_fr_hb && residual && (size_t)M * (size_t)ldo * 2 >= (1ull << 32))
        return fail(DITTO_ERR_SHAPE, "ditto_gemm_ln_bf16: fr_hb needs M * ldo * 2 < 2^32");
    GemmParams p{};
    p.A = (const bf16*)A; p.lda = lda; p.W = (const bf16*)W; p.ldw = K; p.w_rows = N; p.bias = bias;
    p.residual = residual; p.ldr = ldo; p.out = out; p.ldo = ldo; p.M = M; p.N = N; p.K = K;
    if (g_fr_u_fp8 && (N != 1024 || !gamma)) return fail(DITTO_ERR_SHAPE, "fr_u_fp8 (test hook) needs N == 1024 and a LayerNorm output");
    if (g_fr_hb && (N != 768 || g_fr_u_fp8)) return fail(DITTO_ERR_SHAPE, "fr_hb (test hook) needs N == 768 and a bf16 LayerNorm output");
    HIP_TRY(launch_gemm_fr(p, gamma, beta, u_bf16, ldu, g_fr_rot > 1 ? g_fr_rot : 0, (hipStream_t)stream, g_fr_u_fp8 != 0, g_fr_hb != 0));
    return DITTO_OK;
}

int ditto_attention_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                         int B, int H, int Sq, int Skv, int dh, float scale, void* workspace, size_t workspace_bytes,
                         ditto_stream_t stream) {
    if (!q || !k || !v || !out) return fail(DITTO_ERR_ARG, "null pointer to ditto_attention_bf16");
    if (dh % 64) return fail(DITTO_ERR_SHAPE, "head_dim must be a multiple of 64");
    // (head_dim 64: the scratch is OPTIONAL — the split-KV partials of the low-latency class; without it the launch is not split)
    if (dh != 64 && workspace_bytes < attention_workspace_bytes(B, H, Sq, Skv, dh))
        return fail(DITTO_ERR_SIZE, "attention workspace too small");
    AttnArgs a{};
    a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.out_bf16 = out; a.ldo = ldo;
    a.B = B; a.H = H; a.Sq = Sq; a.Skv = Skv; a.dh = dh; a.scale = scale;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    a.q_prescaled = (g_attn_flags & 16) && dh == 64;   // unit tests of the pre-scaled-q kernel: q carries scale*log2(e)
    HIP_TRY(launch_attention(a, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_attention_resid_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid_in,
                               void* resid_out, int ldr, int resid_is_bf16, int B, int H, int Sq, int Skv, int dh, float scale,
                               void* workspace, size_t workspace_bytes, ditto_stream_t stream) {
    if (!q || !k || !v || !resid_out) return fail(DITTO_ERR_ARG, "null pointer to ditto_attention_resid_bf16");
    if (dh % 64) return fail(DITTO_ERR_SHAPE, "head_dim must be a multiple of 64");
    if (ldr < H * dh) return fail(DITTO_ERR_ARG, "ldr must cover H * dh columns");
    if (dh != 64 && workspace_bytes < attention_workspace_bytes(B, H, Sq, Skv, dh))
        return fail(DITTO_ERR_SIZE, "attention workspace too small");
    AttnArgs a{};
    a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv;
    a.resid_f32 = (float*)resid_out; a.ldr = ldr; a.resid_in = (const float*)resid_in; a.resid_bf16 = resid_is_bf16 != 0;
    a.B = B; a.H = H; a.Sq = Sq; a.Skv = Skv; a.dh = dh; a.scale = scale;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    a.q_prescaled = (g_attn_flags & 16) && dh == 64;   // as ditto_attention_bf16
    HIP_TRY(launch_attention(a, (hipStream_t)stream));
    return DITTO_OK;
}

// the operands of the fused head_dim-64 entries (varlen and packed, `layout`): head_dim 64, every leading dimension covering H * 64
// columns in multiples of 8; then the fields of `a` they share (q pre-scaled, no workspace)
static int attn64_args(const char* fn, const char* layout, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                       void* out, int ldo, float* resid_out, const float* resid_in, int ldr, int resid_is_bf16, int B, int H, int dh,
                       AttnArgs& a) {
    if (dh != 64) return fail(DITTO_ERR_SHAPE, "%s: %s attention needs head_dim 64", fn, layout);
    if ((ldq | ldk | ldv) % 8 || ldq < H * dh || ldk < H * dh || ldv < H * dh)
        return fail(DITTO_ERR_SHAPE, "%s: ldq / ldk / ldv must cover H * 64 columns in multiples of 8", fn);
    if (out && (ldo % 8 || ldo < H * dh)) return fail(DITTO_ERR_SHAPE, "%s: ldo must cover H * 64 columns in multiples of 8", fn);
    if (resid_out && (ldr % 8 || ldr < H * dh)) return fail(DITTO_ERR_SHAPE, "%s: ldr must cover H * 64 columns in multiples of 8", fn);
    a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.out_bf16 = out; a.ldo = out ? ldo : 8;
    a.resid_f32 = resid_out; a.ldr = ldr; a.resid_in = resid_in; a.resid_bf16 = resid_is_bf16 != 0;
    a.B = B; a.H = H; a.dh = dh; a.scale = 1.0f; a.q_prescaled = true;
    return DITTO_OK;
}

// variable-length batches: the fused head_dim-64 kernels' VARLEN instantiations (attn64q.h)
static int attention_varlen(const char* fn, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out,
                            int ldo, float* resid_out, const float* resid_in, int ldr, int resid_is_bf16, const int32_t* q_len,
                            const int32_t* kv_len, int B, int H, int Sq, int Skv, int dh, ditto_stream_t stream) {
    if (!q || !k || !v || !(out || resid_out)) return fail(DITTO_ERR_ARG, "%s: null pointer", fn);
    if (B <= 0 || H <= 0 || Sq <= 0 || Skv <= 0) return fail(DITTO_ERR_SHAPE, "%s: B, H, Sq and Skv must be positive", fn);
    AttnArgs a{};
    if (int rc = attn64_args(fn, "variable-length", q, ldq, k, ldk, v, ldv, out, ldo, resid_out, resid_in, ldr, resid_is_bf16, B, H, dh, a))
        return rc;
    a.Sq = Sq; a.Skv = Skv;
    if (!q_len && !kv_len) return fail(DITTO_ERR_ARG, "%s: q_len and kv_len are both NULL (the dense entry serves that)", fn);
    a.q_len = q_len; a.kv_len = kv_len;
    HIP_TRY(launch_attention(a, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_attention_varlen_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                                const int32_t* q_len, const int32_t* kv_len, int B, int H, int Sq, int Skv, int dh,
                                ditto_stream_t stream) {
    if (!out) return fail(DITTO_ERR_ARG, "ditto_attention_varlen_bf16: null pointer");
    return attention_varlen("ditto_attention_varlen_bf16", q, ldq, k, ldk, v, ldv, out, ldo, nullptr, nullptr, 0, 0, q_len,
                            kv_len, B, H, Sq, Skv, dh, stream);
}

int ditto_attention_resid_varlen_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid_in,
                                      void* resid_out, int ldr, int resid_is_bf16, const int32_t* q_len, const int32_t* kv_len,
                                      int B, int H, int Sq, int Skv, int dh, ditto_stream_t stream) {
    if (!resid_out) return fail(DITTO_ERR_ARG, "ditto_attention_resid_varlen_bf16: null pointer");
    return attention_varlen("ditto_attention_resid_varlen_bf16", q, ldq, k, ldk, v, ldv, nullptr, 0, (float*)resid_out,
                            (const float*)resid_in, ldr, resid_is_bf16, q_len, kv_len, B, H, Sq, Skv, dh, stream);
}

// packed batches: the packed instantiations of the fused head_dim-64 kernels (attention_packed.hip)
static int attention_packed(const char* fn, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                            float* resid_out, const float* resid_in, int ldr, int resid_is_bf16, const int32_t* cu_q,
                            const int32_t* cu_kv, int B, int H, int Sq, int Skv, int max_q, int max_kv, int dh, ditto_stream_t stream) {
    if (!q || !k || !v || !(out || resid_out) || !cu_q || !cu_kv) return fail(DITTO_ERR_ARG, "%s: null pointer", fn);
    if (H <= 0) return fail(DITTO_ERR_SHAPE, "%s: H must be positive", fn);
    if (int rc = check_packed(fn, B, Sq, max_q, Skv, max_kv)) return rc;
    AttnArgs a{};
    if (int rc = attn64_args(fn, "packed", q, ldq, k, ldk, v, ldv, out, ldo, resid_out, resid_in, ldr, resid_is_bf16, B, H, dh, a))
        return rc;
    a.Sq = max_q; a.Skv = max_kv;
    a.cu_q = cu_q; a.cu_kv = cu_kv; a.q_rows = Sq; a.kv_rows = Skv;
    HIP_TRY(launch_attention(a, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_attention_packed_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                                const int32_t* cu_q, const int32_t* cu_kv, int B, int H, int Sq, int Skv, int max_q, int max_kv, int dh,
                                ditto_stream_t stream) {
    if (!out) return fail(DITTO_ERR_ARG, "ditto_attention_packed_bf16: null pointer");
    return attention_packed("ditto_attention_packed_bf16", q, ldq, k, ldk, v, ldv, out, ldo, nullptr, nullptr, 0, 0, cu_q, cu_kv, B, H,
                            Sq, Skv, max_q, max_kv, dh, stream);
}

int ditto_attention_resid_packed_bf16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid_in,
                                      void* resid_out, int ldr, int resid_is_bf16, const int32_t* cu_q, const int32_t* cu_kv, int B, int H,
                                      int Sq, int Skv, int max_q, int max_kv, int dh, ditto_stream_t stream) {
    if (!resid_out) return fail(DITTO_ERR_ARG, "ditto_attention_resid_packed_bf16: null pointer");
    return attention_packed("ditto_attention_resid_packed_bf16", q, ldq, k, ldk, v, ldv, nullptr, 0, (float*)resid_out,
                            (const float*)resid_in, ldr, resid_is_bf16, cu_q, cu_kv, B, H, Sq, Skv, max_q, max_kv, dh, stream);
}

int ditto_vq_argmin(const float* latents, const float* codebook, int64_t* idx, int R, int K, int D, float* scratch_k,
                    ditto_stream_t stream) {
    if (!latents || !codebook || !idx || !scratch_k || R <= 0 || K <= 0 || D <= 0)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_vq_argmin");
    HIP_TRY(launch_vq_argmin(latents, codebook, scratch_k, idx, R, K, D, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_embedding_gather(const float* table, const int64_t* ids, float* out, int n, int V, int d,
                           ditto_stream_t stream) {
    if (!table || !ids || !out || n <= 0 || V <= 0 || d <= 0) return fail(DITTO_ERR_ARG, "bad argument to ditto_embedding_gather");
    if (d % 4) return fail(DITTO_ERR_SHAPE, "d must be a multiple of 4");
    HIP_TRY(launch_embedding_gather(table, ids, out, n, V, d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_code_embed_mean(const float* table, const int64_t* codes, float* out, int B, int C, int F, int Fout, int V,
                          int d, ditto_stream_t stream) {
    if (!table || !codes || !out || B <= 0 || C <= 0 || F <= 0 || Fout <= 0 || Fout > F || V <= 0 || d <= 0)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_code_embed_mean");
    if (d % 4) return fail(DITTO_ERR_SHAPE, "d must be a multiple of 4");
    HIP_TRY(launch_code_embed_mean(table, codes, out, B, C, F, Fout, V, d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_linear_update(float* x, const float* eps, const float* noise, const float* a, const float* ce,
                        const float* cz, int B, size_t elems_per_utt, ditto_stream_t stream) {
    if (!x || !eps || !a || !ce || (noise && !cz) || B <= 0 || elems_per_utt == 0)
        return fail(DITTO_ERR_ARG, "bad argument to ditto_linear_update");
    if (elems_per_utt % 4) return fail(DITTO_ERR_SHAPE, "elems_per_utt must be a multiple of 4");
    HIP_TRY(launch_linear_update(x, eps, noise, a, ce, cz, B, elems_per_utt, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_cfg_combine(const float* eps2, float* out, float w, size_t elems_half, ditto_stream_t stream) {
    if (!eps2 || !out || elems_half == 0) return fail(DITTO_ERR_ARG, "bad argument to ditto_cfg_combine");
    if (elems_half % 4) return fail(DITTO_ERR_SHAPE, "elems_half must be a multiple of 4");
    HIP_TRY(launch_cfg_combine(eps2, out, w, elems_half, (hipStream_t)stream));
    return DITTO_OK;
}

// guided strided step (guided.hip): every argument is checked here, before any launch
static int check_guided_update(const char* who, const float* x2, const float* eps2, const float* noise, const int64_t* seeds,
                               const float* w, const float* a, const float* ce, const float* cz, int B, int N, int d, int cfg) {
    if (!x2 || !eps2) return fail(DITTO_ERR_ARG, "%s: null x2 / eps2", who);
    if (noise && seeds) return fail(DITTO_ERR_ARG, "%s: noise and seeds are exclusive (a noise buffer, or Philox from seeds)", who);
    if (cfg && !w) return fail(DITTO_ERR_ARG, "%s: classifier-free guidance needs w (fp32 [B])", who);
    if (!a || !ce || ((noise || seeds) && !cz)) return fail(DITTO_ERR_ARG, "%s: null a / ce / cz", who);
    if (B <= 0 || N <= 0 || d <= 0) return fail(DITTO_ERR_SHAPE, "%s: B, N and d must be positive (B %d, N %d, d %d)", who, B, N, d);
    if (d % 64) return fail(DITTO_ERR_SHAPE, "%s: d %% 64 must be 0 (d %d)", who, d);
    if (B > 65535) return fail(DITTO_ERR_SHAPE, "%s: more than 65535 utterances", who);
    return DITTO_OK;
}

int ditto_guided_update(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                        const float* a, const float* ce, const float* cz, const int32_t* speech_len, int B, int N, int d, int cfg,
                        ditto_stream_t stream) {
    if (int rc = check_guided_update("ditto_guided_update", x2, eps2, noise, seeds, w, a, ce, cz, B, N, d, cfg)) return rc;
    HIP_TRY(launch_guided_update(x2, eps2, noise, seeds, step, w, a, ce, cz, speech_len, B, N, d, cfg != 0, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_guided_step_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* speech_len,
                           const int32_t* text_len, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                           const float* a, const float* ce, const float* cz, int B, int N, int T, int cfg, const float* rope_cos,
                           const float* rope_sin, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                           const ditto_call_opts* opts) {
    if (!m || !cond || !t || !rope_cos || !rope_sin || !workspace) return fail(DITTO_ERR_ARG, "bad argument to ditto_guided_step_opts");
    if (!speech_len != !text_len) return fail(DITTO_ERR_ARG, "ditto_guided_step_opts: speech_len and text_len are both given or both NULL");
    if (T <= 0) return fail(DITTO_ERR_SHAPE, "ditto_guided_step_opts: T must be positive");
    if (int rc = check_guided_update("ditto_guided_step_opts", x2, x2, noise, seeds, w, a, ce, cz, B, N, m->cfg.hidden_dim, cfg))
        return rc;
    return with_opts(opts, [&]() -> int {
        const int nb = cfg ? 2 * B : B;                 // the forward runs over [x; x] x [text; null] under guidance
        float* eps;
        if (int rc = step_forward("ditto_forward", m, x2, cond, t, {rope_cos, rope_sin}, {workspace, workspace_bytes}, stream,
                                  BatchLayout::padded(nb, N, T, speech_len, text_len), &eps))
            return rc;
        ProfScope ps(m, (hipStream_t)stream, DITTO_KC_UPDATE);
        HIP_TRY(launch_guided_update(x2, eps, noise, seeds, step, w, a, ce, cz, speech_len, B, N, m->cfg.hidden_dim, cfg != 0,
                                     (hipStream_t)stream));
        return DITTO_OK;
    });
}

// the packed update (guided_packed.hip) behind the six ditto_guided_update_packed* entries: every argument but an entry's own required
// pointers is checked here, before the launch
static int guided_update_packed_checked(const char* who, float* x2, const float* eps2, const float* noise, const int64_t* seeds,
                                        uint32_t step, const uint32_t* tags, bool per_utt, const float* w, const float* a,
                                        const float* ce, const float* cz, const int32_t* cu, const int32_t* prompt_len,
                                        const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream) {
    if (!cu) return fail(DITTO_ERR_ARG, "%s: null cu", who);
    if (per_utt && seeds && !tags) return fail(DITTO_ERR_ARG, "%s: seeds need tags (uint32 [B])", who);
    if (int rc = check_guided_update(who, x2, eps2, noise, seeds, w, a, ce, cz, B, max_N, d, cfg)) return rc;
    if (int rc = check_packed(who, B, S, max_N, S, max_N)) return rc;
    HIP_TRY(launch_guided_update_packed(x2, eps2, noise, seeds, step, tags, per_utt, w, a, ce, cz, cu, prompt_len, suffix_len, B, S, max_N,
                                        d, cfg != 0, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_guided_update_packed(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                               const float* a, const float* ce, const float* cz, const int32_t* cu, int B, int S, int max_N, int d,
                               int cfg, ditto_stream_t stream) {
    return guided_update_packed_checked("ditto_guided_update_packed", x2, eps2, noise, seeds, step, nullptr, false, w, a, ce, cz, cu,
                                        nullptr, nullptr, B, S, max_N, d, cfg, stream);
}

// ---- guidance rescale (guided_rescale.hip): the scratch [coef_out | scale | partials], each part 256-byte aligned ----
// a step's rescale request: the coefficients to scale are fp32 [B] (coef_in, with w) or ditto_multistep_coef [B] (coefs, w and ke inside)
struct RescaleReq {
    const float* phi; void* scratch; size_t scratch_bytes;
    const float *w, *coef_in; const ditto_multistep_coef* coefs;
    const int32_t *prompt_len, *partner; int G, S_G;   // partner, G, S_G: a mixed step's (else NULL, 0, 0)
};
static size_t rescale_head_bytes(int B) { return al((size_t)B * sizeof(ditto_multistep_coef)) + al((size_t)B * sizeof(float)); }
static size_t rescale_bytes(int B, int max_N, int d) {
    return rescale_head_bytes(B) + al((size_t)B * guidance_rescale_chunks(max_N, d) * 4 * sizeof(double));
}
// every argument of a rescale is checked here, before any launch; coefs != NULL: the ditto_multistep_coef form (w and ke inside)
static int check_rescale(const char* who, const float* eps2, const float* w, const float* phi, const float* coef_in,
                         const ditto_multistep_coef* coefs, const int32_t* cu, const int32_t* partner, int B, int G, int S, int S_G,
                         int max_N, int d, const void* scratch, size_t scratch_bytes) {
    if (!eps2 || !phi || !cu || !scratch) return fail(DITTO_ERR_ARG, "%s: null eps2 / phi / cu / scratch", who);
    if (!coefs == !coef_in) return fail(DITTO_ERR_ARG, "%s: exactly one of coef_in (fp32 [B], with w) and coefs (device [B]) is needed", who);
    if (coef_in && !w) return fail(DITTO_ERR_ARG, "%s: guidance rescale needs w (fp32 [B])", who);
    if ((uintptr_t)coefs % 16) return fail(DITTO_ERR_ARG, "%s: coefs must be 16-byte aligned", who);
    if ((uintptr_t)scratch % 256) return fail(DITTO_ERR_ARG, "%s: the rescale scratch must be 256-byte aligned", who);
    if (d <= 0 || d % 64) return fail(DITTO_ERR_SHAPE, "%s: d %% 64 must be 0 (d %d)", who, d);
    if (int rc = check_packed(who, B, S, max_N, S, max_N)) return rc;
    if (partner && !mixed_layout_ok(B, G, S, S_G))
        return fail(DITTO_ERR_SHAPE, "%s: need 0 <= G <= B, G <= S_G <= S, and S_G == 0 exactly when G == 0 (B %d, G %d, S %d, S_G %d)",
                    who, B, G, S, S_G);
    if (scratch_bytes < rescale_bytes(B, max_N, d))
        return fail(DITTO_ERR_SIZE, "%s: the rescale scratch needs %zu bytes (ditto_guidance_rescale_bytes)", who, rescale_bytes(B, max_N, d));
    return DITTO_OK;
}
static RescaleArgs rescale_args(const float* eps2, const float* w, const float* phi, const float* coef_in,
                                const ditto_multistep_coef* coefs, const int32_t* cu, const int32_t* prompt_len, const int32_t* partner,
                                int B, int G, int S, int S_G, int d, void* scratch, size_t scratch_bytes) {
    RescaleArgs a{};
    char* p = (char*)scratch;
    a.eps2 = eps2; a.phi = phi; a.cu = cu; a.prompt_len = prompt_len; a.partner = partner;
    a.B = B; a.G = G; a.S = S; a.S_G = S_G; a.d = d;
    if (coefs) {   // the whole struct is copied, ke scaled: the per-utterance multistep update reads coefs_out[b]
        a.w = &coefs->w; a.coef_in = &coefs->ke; a.coef_out = &((ditto_multistep_coef*)p)->ke;
        a.cstride = 8; a.koff = 2; a.copy = 8;
    } else {
        a.w = w; a.coef_in = coef_in; a.coef_out = (float*)p;
        a.cstride = 1; a.koff = 0; a.copy = 1;
    }
    a.scale = (float*)(p + al((size_t)B * sizeof(ditto_multistep_coef)));
    a.partial = (double*)(p + rescale_head_bytes(B));
    const size_t slots = (scratch_bytes - rescale_head_bytes(B)) / ((size_t)B * 4 * sizeof(double));
    a.slots = slots > 0x7fffffff ? 0x7fffffff : (int)slots;
    return a;
}

// ---- one guided step over a packed batch: what the 13 ditto_guided_step_packed*_opts entries share, by name ----
struct PackedStep {
    const char* who; ditto_model_t m; float* x2; const void* cond; const int64_t* t;
    const int32_t *cu_speech, *cu_text;
    int B, S, max_N, S_T, max_T;     // the update's: B utterances over the S rows of x
    int nb, rows;                    // the forward's: 2B over 2S, [x; x] x [text; null] (doubled), B + G over S + S_G (mixed), else B over S
    Rope rope; Buf ws; ditto_stream_t stream; const ditto_call_opts* opts;
    // set before B and S are checked (a refused call never reads them), hence the arithmetic that cannot overflow
    void forward_over(bool doubled) { nb = doubled ? (int)(2u * (unsigned)B) : B; rows = doubled ? (int)(2u * (unsigned)S) : S; }
};
// the step entries name these parameters alike: `p` filled from them field by field (nb and rows are the family's to set)
#define PACKED_STEP(p, entry)                                                                                                        \
    PackedStep p{};                                                                                                                  \
    p.who = entry; p.m = m; p.x2 = x2; p.cond = cond; p.t = t; p.cu_speech = cu_speech; p.cu_text = cu_text;                         \
    p.B = B; p.S = S; p.max_N = max_N; p.S_T = S_T; p.max_T = max_T;                                                                 \
    p.rope.cos = rope_cos; p.rope.sin = rope_sin; p.ws.p = workspace; p.ws.bytes = workspace_bytes; p.stream = stream; p.opts = opts

// the one body: check(d), the family's argument checks, refuses before any launch; then the step kernels' limits and check2(d), what
// a family has always checked behind them (a refusal keeps its place); then the forward over p.nb utterances in p.rows rows and
// update(eps, d), the family's launch on the forward's eps
extern "C++" template <class Check, class Check2, class Update>
static int packed_step(const PackedStep& p, Check&& check, Check2&& check2, Update&& update) {
    if (!p.m) return fail(DITTO_ERR_ARG, "bad argument to %s", p.who);
    const int d = p.m->cfg.hidden_dim;
    if (int rc = check(d)) return rc;
    if (p.B > 32767) return fail(DITTO_ERR_SHAPE, "%s: more than 32767 utterances", p.who);
    if (p.S <= 0 || p.S > 0x3fffffff) return fail(DITTO_ERR_SHAPE, "%s: S must lie in [1, 2^30)", p.who);
    if (int rc = check2(d)) return rc;
    return with_opts(p.opts, [&]() -> int {
        float* eps;
        if (int rc = step_forward(p.who, p.m, p.x2, p.cond, p.t, p.rope, p.ws, p.stream,
                                  BatchLayout::packed(p.nb, p.rows, p.max_N, p.S_T, p.max_T, p.cu_speech, p.cu_text), &eps))
            return rc;
        ProfScope ps(p.m, (hipStream_t)p.stream, DITTO_KC_UPDATE);
        return update(eps, d);
    });
}
extern "C++" template <class Check, class Update> static int packed_step(const PackedStep& p, Check&& check, Update&& update) {
    return packed_step(p, check, [](int) { return DITTO_OK; }, update);
}

// guidance rescale inside a step: the request against the step's shapes (before any launch), and the stage between the forward and
// the update — the statistics of this step's eps; returns the scaled coefficients the update reads instead of its own (NULL: failed)
static int check_step_rescale(const PackedStep& p, const RescaleReq& r, int d) {
    return check_rescale(p.who, p.x2, r.w, r.phi, r.coef_in, r.coefs, p.cu_speech, r.partner, p.B, r.G, p.S, r.S_G, p.max_N, d, r.scratch,
                         r.scratch_bytes);
}
static const void* step_rescale(const PackedStep& p, const RescaleReq& r, const float* eps, int d) {
    const RescaleArgs ra = rescale_args(eps, r.w, r.phi, r.coef_in, r.coefs, p.cu_speech, r.prompt_len, r.partner, p.B, r.G, p.S, r.S_G, d,
                                        r.scratch, r.scratch_bytes);
    const hipError_t e = launch_guidance_rescale(ra, p.max_N, (hipStream_t)p.stream);
    if (e != hipSuccess) fail(DITTO_ERR_HIP, "launch_guidance_rescale: %s", hipGetErrorString(e));
    return e == hipSuccess ? r.scratch : nullptr;   // the scratch opens with coef_out, in either form
}

// the strided (DDIM) update of a step: one scalar step tag (per_utt false) or one tag per utterance, over the whole utterance or the
// window that prompt_len and suffix_len (either may be NULL) leave; partner, G, S_G: a mixed step's
struct StridedUpdate {
    const float* noise; const int64_t* seeds; uint32_t step; const uint32_t* tags; bool per_utt;
    const float *w, *a, *ce, *cz; const int32_t *prompt_len, *suffix_len, *partner; int G, S_G, cfg;
    const RescaleReq* rs;            // guidance rescale: the update then reads ce[b] s_b from the scratch
};
static int strided_step(PackedStep& p, const StridedUpdate& u) {
    p.forward_over(u.cfg != 0);      // cu_speech then holds 2B + 1 offsets over 2S rows
    return packed_step(p, [&](int d) -> int {
        if (u.rs)
            if (int rc = check_step_rescale(p, *u.rs, d)) return rc;
        if (int rc = check_guided_update(p.who, p.x2, p.x2, u.noise, u.seeds, u.w, u.a, u.ce, u.cz, p.B, p.max_N, d, u.cfg)) return rc;
        if (u.per_utt && u.seeds && !u.tags) return fail(DITTO_ERR_ARG, "%s: seeds need tags (uint32 [B])", p.who);
        return DITTO_OK;
    }, [&](const float* eps, int d) -> int {
        const float* ce = u.ce;
        if (u.rs && !(ce = (const float*)step_rescale(p, *u.rs, eps, d))) return DITTO_ERR_HIP;
        HIP_TRY(launch_guided_update_packed(p.x2, eps, u.noise, u.seeds, u.step, u.tags, u.per_utt, u.w, u.a, ce, u.cz, p.cu_speech,
                                            u.prompt_len, u.suffix_len, p.B, p.S, p.max_N, d, u.cfg != 0, (hipStream_t)p.stream));
        return DITTO_OK;
    });
}

int ditto_guided_step_packed_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                  const int32_t* cu_text, const float* noise, const int64_t* seeds, uint32_t step, const float* w,
                                  const float* a, const float* ce, const float* cz, int B, int S, int max_N, int S_T, int max_T, int cfg,
                                  const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                  ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_opts");
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.step = step; u.w = w; u.a = a; u.ce = ce; u.cz = cz; u.cfg = cfg;
    return strided_step(p, u);
}

// ---- continuous batching: per-utterance step tags and the device regroup (regroup_packed.hip) ----
int ditto_guided_update_packed_tags(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                    const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu, int B, int S,
                                    int max_N, int d, int cfg, ditto_stream_t stream) {
    return guided_update_packed_checked("ditto_guided_update_packed_tags", x2, eps2, noise, seeds, 0, tags, true, w, a, ce, cz, cu, nullptr,
                                        nullptr, B, S, max_N, d, cfg, stream);
}

int ditto_guided_step_packed_tags_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                       const int32_t* cu_text, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                       const float* w, const float* a, const float* ce, const float* cz, int B, int S, int max_N,
                                       int S_T, int max_T, int cfg, const float* rope_cos, const float* rope_sin, void* workspace,
                                       size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_tags_opts");
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.tags = tags; u.per_utt = true; u.w = w; u.a = a; u.ce = ce; u.cz = cz; u.cfg = cfg;
    return strided_step(p, u);
}

// ---- speech prompts: the packed update and step that leave each utterance's first prompt_len[b] rows alone ----
int ditto_guided_update_packed_prompt(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step,
                                      const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                      const int32_t* prompt_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream) {
    if (!prompt_len) return fail(DITTO_ERR_ARG, "ditto_guided_update_packed_prompt: null prompt_len");
    return guided_update_packed_checked("ditto_guided_update_packed_prompt", x2, eps2, noise, seeds, step, nullptr, false, w, a, ce, cz,
                                        cu, prompt_len, nullptr, B, S, max_N, d, cfg, stream);
}

int ditto_guided_update_packed_tags_prompt(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                           const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                           const int32_t* prompt_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream) {
    if (!prompt_len) return fail(DITTO_ERR_ARG, "ditto_guided_update_packed_tags_prompt: null prompt_len");
    return guided_update_packed_checked("ditto_guided_update_packed_tags_prompt", x2, eps2, noise, seeds, 0, tags, true, w, a, ce, cz, cu,
                                        prompt_len, nullptr, B, S, max_N, d, cfg, stream);
}

int ditto_guided_step_packed_prompt_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                         const int32_t* cu_text, const int32_t* prompt_len, const float* noise, const int64_t* seeds,
                                         uint32_t step, const float* w, const float* a, const float* ce, const float* cz, int B, int S,
                                         int max_N, int S_T, int max_T, int cfg, const float* rope_cos, const float* rope_sin,
                                         void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    if (!prompt_len) return fail(DITTO_ERR_ARG, "ditto_guided_step_packed_prompt_opts: null prompt_len (int32 [B])");
    PACKED_STEP(p, "ditto_guided_step_packed_prompt_opts");
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.step = step; u.w = w; u.a = a; u.ce = ce; u.cz = cz; u.cfg = cfg; u.prompt_len = prompt_len;
    return strided_step(p, u);
}

int ditto_guided_step_packed_tags_prompt_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                              const int32_t* cu_text, const int32_t* prompt_len, const float* noise, const int64_t* seeds,
                                              const uint32_t* tags, const float* w, const float* a, const float* ce, const float* cz,
                                              int B, int S, int max_N, int S_T, int max_T, int cfg, const float* rope_cos,
                                              const float* rope_sin, void* workspace, size_t workspace_bytes, ditto_stream_t stream,
                                              const ditto_call_opts* opts) {
    if (!prompt_len) return fail(DITTO_ERR_ARG, "ditto_guided_step_packed_tags_prompt_opts: null prompt_len (int32 [B])");
    PACKED_STEP(p, "ditto_guided_step_packed_tags_prompt_opts");
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.tags = tags; u.per_utt = true; u.w = w; u.a = a; u.ce = ce; u.cz = cz; u.cfg = cfg;
    u.prompt_len = prompt_len;
    return strided_step(p, u);
}

// ---- the second-order multistep solver over packed batches (guided_multistep.hip) ----
static int check_multistep(const char* who, const float* x2, const float* eps2, const float* q, const ditto_multistep_coef* step,
                           const ditto_multistep_coef* coefs, const float* w, const int32_t* cu, int B, int max_N, int d, int cfg) {
    if (!x2 || !eps2 || !q || !cu) return fail(DITTO_ERR_ARG, "%s: null x2 / eps2 / q / cu", who);
    if (!step == !coefs) return fail(DITTO_ERR_ARG, "%s: exactly one of step (host) and coefs (device [B]) is needed", who);
    if (step && cfg && !w) return fail(DITTO_ERR_ARG, "%s: classifier-free guidance needs w (fp32 [B])", who);
    if ((uintptr_t)coefs % 16) return fail(DITTO_ERR_ARG, "%s: coefs must be 16-byte aligned", who);
    if (B <= 0 || max_N <= 0 || d <= 0) return fail(DITTO_ERR_SHAPE, "%s: B, max_N and d must be positive (B %d, max_N %d, d %d)", who, B, max_N, d);
    if (d % 64) return fail(DITTO_ERR_SHAPE, "%s: d %% 64 must be 0 (d %d)", who, d);
    if (B > 65535) return fail(DITTO_ERR_SHAPE, "%s: more than 65535 utterances", who);
    return DITTO_OK;
}

static int multistep_update_checked(const char* who, float* x2, const float* eps2, float* q, const ditto_multistep_coef* step,
                                    const ditto_multistep_coef* coefs, const float* w, const int32_t* cu, const int32_t* prompt_len,
                                    const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream) {
    if (int rc = check_multistep(who, x2, eps2, q, step, coefs, w, cu, B, max_N, d, cfg)) return rc;
    if (int rc = check_packed(who, B, S, max_N, S, max_N)) return rc;
    HIP_TRY(launch_multistep_update_packed(x2, eps2, q, step, coefs, w, cu, prompt_len, suffix_len, B, S, max_N, d, cfg != 0,
                                           (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_multistep_update_packed(float* x2, const float* eps2, float* q, const ditto_multistep_coef* step,
                                  const ditto_multistep_coef* coefs, const float* w, const int32_t* cu, const int32_t* prompt_len,
                                  int B, int S, int max_N, int d, int cfg, ditto_stream_t stream) {
    return multistep_update_checked("ditto_multistep_update_packed", x2, eps2, q, step, coefs, w, cu, prompt_len, nullptr, B, S, max_N, d,
                                    cfg, stream);
}

// the multistep update of a step, over the forward of strided_step: [x; x] x [text; null] under guidance
struct MultistepUpdate {
    float* q; const ditto_multistep_coef *step, *coefs; const float* w; const int32_t *prompt_len, *suffix_len; int cfg;
    const RescaleReq* rs;            // guidance rescale: the per-utterance update then reads ke[b] s_b from the scratch's copy of coefs
};
static int multistep_step(PackedStep& p, const MultistepUpdate& u) {
    p.forward_over(u.cfg != 0);
    return packed_step(p, [&](int d) -> int {
        return check_multistep(p.who, p.x2, p.x2, u.q, u.step, u.coefs, u.w, p.cu_speech, p.B, p.max_N, d, u.cfg);
    }, [&](int d) -> int {
        return u.rs ? check_step_rescale(p, *u.rs, d) : DITTO_OK;
    }, [&](const float* eps, int d) -> int {
        const ditto_multistep_coef* coefs = u.coefs;
        if (u.rs && !(coefs = (const ditto_multistep_coef*)step_rescale(p, *u.rs, eps, d))) return DITTO_ERR_HIP;
        HIP_TRY(launch_multistep_update_packed(p.x2, eps, u.q, u.step, coefs, u.w, p.cu_speech, u.prompt_len, u.suffix_len, p.B, p.S,
                                               p.max_N, d, u.cfg != 0, (hipStream_t)p.stream));
        return DITTO_OK;
    });
}

int ditto_guided_step_packed_multistep_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                            const int32_t* cu_text, const int32_t* prompt_len, float* q,
                                            const ditto_multistep_coef* step, const ditto_multistep_coef* coefs, const float* w, int B,
                                            int S, int max_N, int S_T, int max_T, int cfg, const float* rope_cos, const float* rope_sin,
                                            void* workspace, size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_multistep_opts");
    MultistepUpdate u{};
    u.q = q; u.step = step; u.coefs = coefs; u.w = w; u.prompt_len = prompt_len; u.cfg = cfg;
    return multistep_step(p, u);
}

// ---- guidance in a limited interval: a step in which G of the B utterances are guided (guided_mixed.hip) ----
static int check_mixed(const char* who, const float* x2, const float* eps2, const float* noise, const int64_t* seeds,
                       const uint32_t* tags, const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                       const int32_t* partner, int B, int G, int S, int S_G, int max_N, int d) {
    if (!cu || !partner) return fail(DITTO_ERR_ARG, "%s: null cu / partner", who);
    if (seeds && !tags) return fail(DITTO_ERR_ARG, "%s: seeds need tags (uint32 [B])", who);
    if (int rc = check_guided_update(who, x2, eps2, noise, seeds, w, a, ce, cz, B, max_N, d, 1)) return rc;
    if (int rc = check_packed(who, B, S, max_N, S, max_N)) return rc;
    if (!mixed_layout_ok(B, G, S, S_G))
        return fail(DITTO_ERR_SHAPE, "%s: need 0 <= G <= B, G <= S_G <= S, and S_G == 0 exactly when G == 0 (B %d, G %d, S %d, S_G %d)",
                    who, B, G, S, S_G);
    return DITTO_OK;
}

int ditto_guided_update_packed_mixed(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                     const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                     const int32_t* partner, const int32_t* prompt_len, int B, int G, int S, int S_G, int max_N, int d,
                                     ditto_stream_t stream) {
    if (int rc = check_mixed("ditto_guided_update_packed_mixed", x2, eps2, noise, seeds, tags, w, a, ce, cz, cu, partner, B, G, S, S_G,
                             max_N, d))
        return rc;
    HIP_TRY(launch_guided_update_mixed(x2, eps2, noise, seeds, tags, w, a, ce, cz, cu, partner, prompt_len, B, G, S, S_G, max_N, d,
                                       (hipStream_t)stream));
    return DITTO_OK;
}

// the mixed step: the forward over [x; the guided ones' copies] x [text; their null], the tagged strided update over partner
static int mixed_step(PackedStep& p, const StridedUpdate& u) {
    return packed_step(p, [&](int d) -> int {
        if (int rc = check_mixed(p.who, p.x2, p.x2, u.noise, u.seeds, u.tags, u.w, u.a, u.ce, u.cz, p.cu_speech, u.partner, p.B, u.G, p.S,
                                 u.S_G, p.max_N, d))
            return rc;
        p.nb = p.B + u.G; p.rows = p.S + u.S_G;   // G <= B and S_G <= S from here on
        return DITTO_OK;
    }, [&](int d) -> int {
        return u.rs ? check_step_rescale(p, *u.rs, d) : DITTO_OK;
    }, [&](const float* eps, int d) -> int {
        const float* ce = u.ce;
        if (u.rs && !(ce = (const float*)step_rescale(p, *u.rs, eps, d))) return DITTO_ERR_HIP;
        HIP_TRY(launch_guided_update_mixed(p.x2, eps, u.noise, u.seeds, u.tags, u.w, u.a, ce, u.cz, p.cu_speech, u.partner, u.prompt_len,
                                           p.B, u.G, p.S, u.S_G, p.max_N, d, (hipStream_t)p.stream));
        return DITTO_OK;
    });
}

int ditto_guided_step_packed_mixed_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                        const int32_t* cu_text, const int32_t* partner, const int32_t* prompt_len, const float* noise,
                                        const int64_t* seeds, const uint32_t* tags, const float* w, const float* a, const float* ce,
                                        const float* cz, int B, int G, int S, int S_G, int max_N, int S_T, int max_T,
                                        const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                        ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_mixed_opts");
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.tags = tags; u.w = w; u.a = a; u.ce = ce; u.cz = cz;
    u.prompt_len = prompt_len; u.partner = partner; u.G = G; u.S_G = S_G;
    return mixed_step(p, u);
}

// ---- guidance rescale (Lin et al. 2024, section 3.4; guided_rescale.hip): the statistics alone, and the steps that use them ----
size_t ditto_guidance_rescale_bytes(int B, int max_N, int d) {
    if (B <= 0 || max_N <= 0 || d <= 0 || d % 64) {
        fail(DITTO_ERR_SHAPE, "ditto_guidance_rescale_bytes: B and max_N must be positive and d %% 64 == 0");
        return 0;
    }
    return rescale_bytes(B, max_N, d);
}

int ditto_guidance_rescale_packed(const float* eps2, const float* w, const float* phi, const float* coef_in,
                                  const ditto_multistep_coef* coefs, const int32_t* cu, const int32_t* prompt_len, const int32_t* partner,
                                  int B, int G, int S, int S_G, int max_N, int d, void* scratch, size_t scratch_bytes,
                                  ditto_stream_t stream) {
    if (int rc = check_rescale("ditto_guidance_rescale_packed", eps2, w, phi, coef_in, coefs, cu, partner, B, G, S, S_G, max_N, d, scratch,
                               scratch_bytes))
        return rc;
    const RescaleArgs ra = rescale_args(eps2, w, phi, coef_in, coefs, cu, prompt_len, partner, B, G, S, S_G, d, scratch, scratch_bytes);
    HIP_TRY(launch_guidance_rescale(ra, max_N, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_guided_step_packed_rescale_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                          const int32_t* cu_text, const int32_t* partner, const int32_t* prompt_len, const float* noise,
                                          const int64_t* seeds, uint32_t step, const uint32_t* tags, const float* w, const float* phi,
                                          const float* a, const float* ce, const float* cz, int B, int G, int S, int S_G, int max_N,
                                          int S_T, int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                          size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                          const ditto_call_opts* opts) {
    const char* who = "ditto_guided_step_packed_rescale_opts";
    if (!w) return fail(DITTO_ERR_ARG, "%s: guidance rescale needs w (fp32 [B])", who);
    PACKED_STEP(p, who);
    RescaleReq rs{};
    rs.phi = phi; rs.scratch = scratch; rs.scratch_bytes = scratch_bytes; rs.w = w; rs.coef_in = ce; rs.prompt_len = prompt_len;
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.step = step; u.tags = tags; u.per_utt = tags != nullptr; u.w = w; u.a = a; u.ce = ce; u.cz = cz;
    u.cfg = 1; u.prompt_len = prompt_len; u.rs = &rs;
    if (!partner) return strided_step(p, u);
    rs.partner = u.partner = partner; rs.G = u.G = G; rs.S_G = u.S_G = S_G;   // some utterances guided: the mixed entry's forward and update
    return mixed_step(p, u);
}

int ditto_guided_step_packed_multistep_rescale_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                    const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len, float* q,
                                                    const ditto_multistep_coef* coefs, const float* phi, int B, int S, int max_N, int S_T,
                                                    int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                                    size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                                    const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_multistep_rescale_opts");
    RescaleReq rs{};
    rs.phi = phi; rs.scratch = scratch; rs.scratch_bytes = scratch_bytes; rs.coefs = coefs; rs.prompt_len = prompt_len;
    MultistepUpdate u{};
    u.q = q; u.coefs = coefs; u.prompt_len = prompt_len; u.cfg = 1; u.rs = &rs;
    return multistep_step(p, u);
}

// ---- span-masked training over a packed batch (span_train.hip): the span behind a prompt, or a window with context on both sides ----
static int check_span(const char* who, const void* in, const float* noise, const int64_t* seeds, const int32_t* cu, const void* out, int B,
                      int S, int max_N, int d) {
    if (!in || !out || !cu) return fail(DITTO_ERR_ARG, "%s: null pointer", who);
    if (!noise == !seeds) return fail(DITTO_ERR_ARG, "%s: exactly one of noise (a packed buffer) and seeds (Philox) is needed", who);
    if (d <= 0 || d % 64) return fail(DITTO_ERR_SHAPE, "%s: d %% 64 must be 0 (d %d)", who, d);
    return check_packed(who, B, S, max_N, S, max_N);
}

static int span_noise_checked(const char* who, const float* x0, const float* noise, const int64_t* seeds, uint32_t tag, const float* ca,
                              const float* cs, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, float* x_in, int B,
                              int S, int max_N, int d, ditto_stream_t stream) {
    if (!ca || !cs) return fail(DITTO_ERR_ARG, "%s: null ca / cs", who);
    if (int rc = check_span(who, x0, noise, seeds, cu, x_in, B, S, max_N, d)) return rc;
    HIP_TRY(launch_span_noise_packed(x0, noise, seeds, tag, ca, cs, cu, prompt_len, suffix_len, x_in, B, S, max_N, d, (hipStream_t)stream));
    return DITTO_OK;
}

static int span_mse_checked(const char* who, const float* eps, const float* noise, const int64_t* seeds, uint32_t tag, const int32_t* cu,
                            const int32_t* prompt_len, const int32_t* suffix_len, size_t n_elems, float* grad_eps, float* loss,
                            void* workspace, size_t workspace_bytes, int B, int S, int max_N, int d, ditto_stream_t stream) {
    if (!loss || !workspace) return fail(DITTO_ERR_ARG, "%s: null loss / workspace", who);
    if (int rc = check_span(who, eps, noise, seeds, cu, grad_eps, B, S, max_N, d)) return rc;
    if (n_elems == 0 || n_elems > (size_t)S * d) return fail(DITTO_ERR_SHAPE, "%s: n_elems must lie in [1, S d]", who);
    if ((uintptr_t)workspace % 4 || workspace_bytes < span_mse_partials(B, max_N, d) * sizeof(float))
        return fail(DITTO_ERR_SIZE, "%s: the workspace needs %zu bytes (B x min(1024, ceil(max_N d / 1024)) floats)", who,
                    span_mse_partials(B, max_N, d) * sizeof(float));
    HIP_TRY(launch_span_mse_packed(eps, noise, seeds, tag, cu, prompt_len, suffix_len, (double)n_elems, grad_eps, loss, (float*)workspace,
                                   B, S, max_N, d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_span_noise_packed(const float* x0, const float* noise, const int64_t* seeds, uint32_t tag, const float* ca, const float* cs,
                            const int32_t* cu, const int32_t* prompt_len, float* x_in, int B, int S, int max_N, int d,
                            ditto_stream_t stream) {
    if (!prompt_len) return fail(DITTO_ERR_ARG, "ditto_span_noise_packed: null prompt_len");
    return span_noise_checked("ditto_span_noise_packed", x0, noise, seeds, tag, ca, cs, cu, prompt_len, nullptr, x_in, B, S, max_N, d,
                              stream);
}

int ditto_span_mse_packed(const float* eps, const float* noise, const int64_t* seeds, uint32_t tag, const int32_t* cu,
                          const int32_t* prompt_len, size_t n_elems, float* grad_eps, float* loss, void* workspace,
                          size_t workspace_bytes, int B, int S, int max_N, int d, ditto_stream_t stream) {
    if (!prompt_len) return fail(DITTO_ERR_ARG, "ditto_span_mse_packed: null prompt_len");
    return span_mse_checked("ditto_span_mse_packed", eps, noise, seeds, tag, cu, prompt_len, nullptr, n_elems, grad_eps, loss, workspace,
                            workspace_bytes, B, S, max_N, d, stream);
}

int ditto_span_noise_window(const float* x0, const float* noise, const int64_t* seeds, uint32_t tag, const float* ca, const float* cs,
                            const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, float* x_in, int B, int S,
                            int max_N, int d, ditto_stream_t stream) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_span_noise_window: null suffix_len");
    return span_noise_checked("ditto_span_noise_window", x0, noise, seeds, tag, ca, cs, cu, prompt_len, suffix_len, x_in, B, S, max_N, d,
                              stream);
}

int ditto_span_mse_window(const float* eps, const float* noise, const int64_t* seeds, uint32_t tag, const int32_t* cu,
                          const int32_t* prompt_len, const int32_t* suffix_len, size_t n_elems, float* grad_eps, float* loss,
                          void* workspace, size_t workspace_bytes, int B, int S, int max_N, int d, ditto_stream_t stream) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_span_mse_window: null suffix_len");
    return span_mse_checked("ditto_span_mse_window", eps, noise, seeds, tag, cu, prompt_len, suffix_len, n_elems, grad_eps, loss, workspace,
                            workspace_bytes, B, S, max_N, d, stream);
}

int ditto_span_vloss_window(const float* pred, const float* x0, const float* noise, const int64_t* seeds, uint32_t tag, const float* ca,
                            const float* cs, const float* lw, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len,
                            size_t n_elems, float* grad_pred, float* loss, void* workspace, size_t workspace_bytes, int B, int S,
                            int max_N, int d, ditto_stream_t stream) {
    const char* who = "ditto_span_vloss_window";
    if (!loss || !workspace) return fail(DITTO_ERR_ARG, "%s: null loss / workspace", who);
    if (!x0 || !ca || !cs) return fail(DITTO_ERR_ARG, "%s: null x0 / ca / cs", who);
    if (int rc = check_span(who, pred, noise, seeds, cu, grad_pred, B, S, max_N, d)) return rc;
    if (n_elems == 0 || n_elems > (size_t)S * d) return fail(DITTO_ERR_SHAPE, "%s: n_elems must lie in [1, S d]", who);
    if ((uintptr_t)workspace % 4 || workspace_bytes < span_mse_partials(B, max_N, d) * sizeof(float))
        return fail(DITTO_ERR_SIZE, "%s: the workspace needs %zu bytes (B x min(1024, ceil(max_N d / 1024)) floats)", who,
                    span_mse_partials(B, max_N, d) * sizeof(float));
    HIP_TRY(launch_span_vloss_packed(pred, x0, noise, seeds, tag, ca, cs, lw, cu, prompt_len, suffix_len, (double)n_elems, grad_pred, loss,
                                     (float*)workspace, B, S, max_N, d, (hipStream_t)stream));
    return DITTO_OK;
}

// ---- speech infilling: the update and step entries over the window [cu[b] + P_b, cu[b+1] - Q_b) ----
int ditto_guided_update_packed_window(float* x2, const float* eps2, const float* noise, const int64_t* seeds, uint32_t step,
                                      const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                      const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg,
                                      ditto_stream_t stream) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_guided_update_packed_window: null suffix_len");
    return guided_update_packed_checked("ditto_guided_update_packed_window", x2, eps2, noise, seeds, step, nullptr, false, w, a, ce, cz,
                                        cu, prompt_len, suffix_len, B, S, max_N, d, cfg, stream);
}

int ditto_guided_update_packed_tags_window(float* x2, const float* eps2, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                           const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                           const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg,
                                           ditto_stream_t stream) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_guided_update_packed_tags_window: null suffix_len");
    return guided_update_packed_checked("ditto_guided_update_packed_tags_window", x2, eps2, noise, seeds, 0, tags, true, w, a, ce, cz, cu,
                                        prompt_len, suffix_len, B, S, max_N, d, cfg, stream);
}

int ditto_guided_step_packed_window_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                         const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len,
                                         const float* noise, const int64_t* seeds, uint32_t step, const float* w, const float* a,
                                         const float* ce, const float* cz, int B, int S, int max_N, int S_T, int max_T, int cfg,
                                         const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                         ditto_stream_t stream, const ditto_call_opts* opts) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_guided_step_packed_window_opts: null suffix_len (int32 [B])");
    PACKED_STEP(p, "ditto_guided_step_packed_window_opts");
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.step = step; u.w = w; u.a = a; u.ce = ce; u.cz = cz; u.cfg = cfg;
    u.prompt_len = prompt_len; u.suffix_len = suffix_len;
    return strided_step(p, u);
}

int ditto_guided_step_packed_tags_window_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                              const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len,
                                              const float* noise, const int64_t* seeds, const uint32_t* tags, const float* w,
                                              const float* a, const float* ce, const float* cz, int B, int S, int max_N, int S_T,
                                              int max_T, int cfg, const float* rope_cos, const float* rope_sin, void* workspace,
                                              size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_guided_step_packed_tags_window_opts: null suffix_len (int32 [B])");
    PACKED_STEP(p, "ditto_guided_step_packed_tags_window_opts");
    StridedUpdate u{};
    u.noise = noise; u.seeds = seeds; u.tags = tags; u.per_utt = true; u.w = w; u.a = a; u.ce = ce; u.cz = cz; u.cfg = cfg;
    u.prompt_len = prompt_len; u.suffix_len = suffix_len;
    return strided_step(p, u);
}

int ditto_multistep_update_window(float* x2, const float* eps2, float* q, const ditto_multistep_coef* step,
                                  const ditto_multistep_coef* coefs, const float* w, const int32_t* cu, const int32_t* prompt_len,
                                  const int32_t* suffix_len, int B, int S, int max_N, int d, int cfg, ditto_stream_t stream) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_multistep_update_window: null suffix_len");
    return multistep_update_checked("ditto_multistep_update_window", x2, eps2, q, step, coefs, w, cu, prompt_len, suffix_len, B, S, max_N,
                                    d, cfg, stream);
}

int ditto_guided_step_packed_multistep_window_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                   const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len,
                                                   const int32_t* suffix_len, float* q, const ditto_multistep_coef* step,
                                                   const ditto_multistep_coef* coefs, const float* w, int B, int S, int max_N, int S_T,
                                                   int max_T, int cfg, const float* rope_cos, const float* rope_sin, void* workspace,
                                                   size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    if (!suffix_len) return fail(DITTO_ERR_ARG, "ditto_guided_step_packed_multistep_window_opts: null suffix_len (int32 [B])");
    PACKED_STEP(p, "ditto_guided_step_packed_multistep_window_opts");
    MultistepUpdate u{};
    u.q = q; u.step = step; u.coefs = coefs; u.w = w; u.prompt_len = prompt_len; u.suffix_len = suffix_len; u.cfg = cfg;
    return multistep_step(p, u);
}

// ---- guidance reuse (guided_reuse.hip): every argument is checked here, before any launch ----
static int check_reuse(const char* who, const float* delta, const float* w, const int32_t* cu, int B, int S, int max_N, int mode,
                       int mirror) {
    if (!delta) return fail(DITTO_ERR_ARG, "%s: null delta (fp32 [S, d])", who);
    if (!cu) return fail(DITTO_ERR_ARG, "%s: null cu", who);
    if (!w) return fail(DITTO_ERR_ARG, "%s: guidance reuse needs w (fp32 [B])", who);
    if (mode != 1 && mode != 2) return fail(DITTO_ERR_ARG, "%s: mode must be 1 (STORE) or 2 (LOAD), not %d", who, mode);
    if (mode == 1 && mirror) return fail(DITTO_ERR_ARG, "%s: mirror belongs to LOAD (STORE writes both halves anyway)", who);
    return check_packed(who, B, S, max_N, S, max_N);
}

int ditto_guided_update_packed_reuse(float* x2, const float* eps, float* delta, const float* noise, const int64_t* seeds, uint32_t step,
                                     const float* w, const float* a, const float* ce, const float* cz, const int32_t* cu,
                                     const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, int mode,
                                     int mirror, ditto_stream_t stream) {
    const char* who = "ditto_guided_update_packed_reuse";
    if (int rc = check_guided_update(who, x2, eps, noise, seeds, w, a, ce, cz, B, max_N, d, 1)) return rc;
    if (int rc = check_reuse(who, delta, w, cu, B, S, max_N, mode, mirror)) return rc;
    HIP_TRY(launch_guided_update_reuse(x2, eps, delta, noise, seeds, step, w, a, ce, cz, cu, prompt_len, suffix_len, B, S, max_N, d, mode,
                                       mirror, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_multistep_update_packed_reuse(float* x2, const float* eps, float* q, float* delta, const ditto_multistep_coef* step,
                                        const float* w, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                        int S, int max_N, int d, int mode, int mirror, ditto_stream_t stream) {
    const char* who = "ditto_multistep_update_packed_reuse";
    if (!step) return fail(DITTO_ERR_ARG, "%s: null step (host ditto_multistep_coef)", who);
    if (int rc = check_multistep(who, x2, eps, q, step, nullptr, w, cu, B, max_N, d, 1)) return rc;
    if (int rc = check_reuse(who, delta, w, cu, B, S, max_N, mode, mirror)) return rc;
    HIP_TRY(launch_multistep_update_reuse(x2, eps, q, delta, step, w, cu, prompt_len, suffix_len, B, S, max_N, d, mode, mirror,
                                          (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_guided_step_packed_reuse_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                        const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len, float* delta,
                                        const float* noise, const int64_t* seeds, uint32_t step, const float* w, const float* a,
                                        const float* ce, const float* cz, int B, int S, int max_N, int S_T, int max_T, int mode,
                                        int mirror, const float* rope_cos, const float* rope_sin, void* workspace,
                                        size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_reuse_opts");
    p.forward_over(mode == 1);
    return packed_step(p, [&](int d) -> int {
        if (int rc = check_guided_update(p.who, x2, x2, noise, seeds, w, a, ce, cz, B, max_N, d, 1)) return rc;
        return check_reuse(p.who, delta, w, cu_speech, B, S, max_N, mode, mirror);
    }, [&](const float* eps, int d) -> int {
        HIP_TRY(launch_guided_update_reuse(x2, eps, delta, noise, seeds, step, w, a, ce, cz, cu_speech, prompt_len, suffix_len, B, S, max_N,
                                           d, mode, mirror, (hipStream_t)stream));
        return DITTO_OK;
    });
}

int ditto_guided_step_packed_multistep_reuse_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                  const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len,
                                                  const int32_t* suffix_len, float* q, float* delta, const ditto_multistep_coef* step,
                                                  const float* w, int B, int S, int max_N, int S_T, int max_T, int mode, int mirror,
                                                  const float* rope_cos, const float* rope_sin, void* workspace, size_t workspace_bytes,
                                                  ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_multistep_reuse_opts");
    p.forward_over(mode == 1);
    return packed_step(p, [&](int d) -> int {
        if (!step) return fail(DITTO_ERR_ARG, "%s: null step (host ditto_multistep_coef)", p.who);
        if (int rc = check_multistep(p.who, x2, x2, q, step, nullptr, w, cu_speech, B, max_N, d, 1)) return rc;
        return check_reuse(p.who, delta, w, cu_speech, B, S, max_N, mode, mirror);
    }, [&](const float* eps, int d) -> int {
        HIP_TRY(launch_multistep_update_reuse(x2, eps, q, delta, step, w, cu_speech, prompt_len, suffix_len, B, S, max_N, d, mode, mirror,
                                              (hipStream_t)stream));
        return DITTO_OK;
    });
}

// ---- guidance reuse in a request stream (guided_refresh.hip; include/ditto_refresh.h): a step of refreshing, reusing and plain utterances ----
static int check_refresh(const char* who, const float* x2, const float* eps2, const float* delta, const float* noise,
                         const int64_t* seeds, const uint32_t* tags, const float* w, const float* a, const float* ce, const float* cz,
                         const int32_t* cu, const int32_t* partner, const int32_t* kind, int B, int G, int S, int S_G, int max_N, int d) {
    if (!delta) return fail(DITTO_ERR_ARG, "%s: null delta (fp32 [S, d])", who);
    if (!kind) return fail(DITTO_ERR_ARG, "%s: null kind (int32 [B])", who);
    return check_mixed(who, x2, eps2, noise, seeds, tags, w, a, ce, cz, cu, partner, B, G, S, S_G, max_N, d);
}

int ditto_guided_update_packed_refresh(float* x2, const float* eps2, float* delta, const float* noise, const int64_t* seeds,
                                       const uint32_t* tags, const float* w, const float* a, const float* ce, const float* cz,
                                       const int32_t* cu, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len, int B,
                                       int G, int S, int S_G, int max_N, int d, ditto_stream_t stream) {
    if (int rc = check_refresh("ditto_guided_update_packed_refresh", x2, eps2, delta, noise, seeds, tags, w, a, ce, cz, cu, partner, kind,
                               B, G, S, S_G, max_N, d))
        return rc;
    HIP_TRY(launch_guided_update_refresh(x2, eps2, delta, noise, seeds, tags, w, a, ce, cz, cu, partner, kind, prompt_len, B, G, S, S_G,
                                         max_N, d, (hipStream_t)stream));
    return DITTO_OK;
}

// the mixed step's forward — over [x; the refreshing ones' copies] x [text; their null], over the B utterances alone when G == 0 —
// then the three-kind update
int ditto_guided_step_packed_refresh_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                          const int32_t* cu_text, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len,
                                          float* delta, const float* noise, const int64_t* seeds, const uint32_t* tags, const float* w,
                                          const float* a, const float* ce, const float* cz, int B, int G, int S, int S_G, int max_N,
                                          int S_T, int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                          size_t workspace_bytes, ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_refresh_opts");
    return packed_step(p, [&](int d) -> int {
        if (int rc = check_refresh(p.who, x2, x2, delta, noise, seeds, tags, w, a, ce, cz, cu_speech, partner, kind, B, G, S, S_G, max_N, d))
            return rc;
        p.nb = B + G; p.rows = S + S_G;   // G <= B and S_G <= S from here on
        return DITTO_OK;
    }, [&](const float* eps, int d) -> int {
        HIP_TRY(launch_guided_update_refresh(x2, eps, delta, noise, seeds, tags, w, a, ce, cz, cu_speech, partner, kind, prompt_len, B, G, S,
                                             S_G, max_N, d, (hipStream_t)stream));
        return DITTO_OK;
    });
}

// ---- projected guidance (APG, Sadat et al. 2024; guided_project.hip; include/ditto_project.h): the scratch [pcoef | partials], each
// part 256-byte aligned; the statistics alone, the two updates, and the steps that chain them behind the forward ----
static size_t project_head_bytes(int B) { return al((size_t)B * 4 * sizeof(float)); }
static size_t project_bytes(int B, int max_N, int d) {
    return project_head_bytes(B) + al((size_t)B * guidance_rescale_chunks(max_N, d) * 4 * sizeof(double));
}
// what every project entry shares: the rows, the shapes and cu
static int check_project_rows(const char* who, const float* x2, const float* eps2, const float* dir, const int32_t* cu, int B, int S,
                              int max_N, int d) {
    if (!x2 || !eps2 || !dir || !cu) return fail(DITTO_ERR_ARG, "%s: null x2 / eps2 / dir / cu", who);
    if (((uintptr_t)x2 | (uintptr_t)eps2 | (uintptr_t)dir) % 16) return fail(DITTO_ERR_ARG, "%s: x2, eps2 and dir must be 16-byte aligned", who);
    if (d <= 0 || d % 64) return fail(DITTO_ERR_SHAPE, "%s: d %% 64 must be 0 (d %d)", who, d);
    return check_packed(who, B, S, max_N, S, max_N);
}
// every argument of launch 1 and the finish is checked here, before any launch
static int check_project(const char* who, const float* x2, const float* eps2, const float* dir, const ditto_project_coef* proj,
                         const int32_t* cu, int B, int S, int max_N, int d, const void* scratch, size_t scratch_bytes) {
    if (!proj || !scratch) return fail(DITTO_ERR_ARG, "%s: null proj / scratch", who);
    if ((uintptr_t)proj % 16) return fail(DITTO_ERR_ARG, "%s: proj must be 16-byte aligned", who);
    if ((uintptr_t)scratch % 256) return fail(DITTO_ERR_ARG, "%s: the project scratch must be 256-byte aligned", who);
    if (int rc = check_project_rows(who, x2, eps2, dir, cu, B, S, max_N, d)) return rc;
    if (scratch_bytes < project_bytes(B, max_N, d))
        return fail(DITTO_ERR_SIZE, "%s: the project scratch needs %zu bytes (ditto_guidance_project_bytes)", who, project_bytes(B, max_N, d));
    return DITTO_OK;
}
static ProjectArgs project_args(const float* x2, const float* eps2, float* dir, const ditto_project_coef* proj, const int32_t* cu,
                                const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int d, void* scratch,
                                size_t scratch_bytes) {
    ProjectArgs a{};
    a.x2 = x2; a.eps2 = eps2; a.dir = dir; a.proj = proj; a.cu = cu; a.prompt_len = prompt_len; a.suffix_len = suffix_len;
    a.B = B; a.S = S; a.d = d;
    a.pcoef = (float*)scratch;
    a.partial = (double*)((char*)scratch + project_head_bytes(B));
    const size_t slots = (scratch_bytes - project_head_bytes(B)) / ((size_t)B * 4 * sizeof(double));
    a.slots = slots > 0x7fffffff ? 0x7fffffff : (int)slots;
    return a;
}
static int check_project_ddim(const char* who, const float* pcoef, const float* noise, const int64_t* seeds, const float* a,
                              const float* ce, const float* cz) {
    if (!pcoef || (uintptr_t)pcoef % 16) return fail(DITTO_ERR_ARG, "%s: pcoef (fp32 [B, 4]) must be given and 16-byte aligned", who);
    if (noise && seeds) return fail(DITTO_ERR_ARG, "%s: noise and seeds are exclusive (a noise buffer, or Philox from seeds)", who);
    if ((uintptr_t)noise % 16) return fail(DITTO_ERR_ARG, "%s: noise must be 16-byte aligned", who);
    if (!a || !ce || ((noise || seeds) && !cz)) return fail(DITTO_ERR_ARG, "%s: null a / ce / cz", who);
    return DITTO_OK;
}
static int check_project_multistep(const char* who, const float* pcoef, const float* q, const ditto_multistep_coef* step,
                                   const ditto_multistep_coef* coefs) {
    if (!pcoef || (uintptr_t)pcoef % 16) return fail(DITTO_ERR_ARG, "%s: pcoef (fp32 [B, 4]) must be given and 16-byte aligned", who);
    if (!q || (uintptr_t)q % 16) return fail(DITTO_ERR_ARG, "%s: q (fp32 [S, d]) must be given and 16-byte aligned", who);
    if (!step == !coefs) return fail(DITTO_ERR_ARG, "%s: exactly one of step (host) and coefs (device [B]) is needed", who);
    if ((uintptr_t)coefs % 16) return fail(DITTO_ERR_ARG, "%s: coefs must be 16-byte aligned", who);
    return DITTO_OK;
}

size_t ditto_guidance_project_bytes(int B, int max_N, int d) {
    if (B <= 0 || max_N <= 0 || d <= 0 || d % 64) {
        fail(DITTO_ERR_SHAPE, "ditto_guidance_project_bytes: B and max_N must be positive and d %% 64 == 0");
        return 0;
    }
    return project_bytes(B, max_N, d);
}

int ditto_guidance_project_packed(const float* x2, const float* eps2, float* dir, const ditto_project_coef* proj, const int32_t* cu,
                                  const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d, void* scratch,
                                  size_t scratch_bytes, ditto_stream_t stream) {
    if (int rc = check_project("ditto_guidance_project_packed", x2, eps2, dir, proj, cu, B, S, max_N, d, scratch, scratch_bytes)) return rc;
    HIP_TRY(launch_guidance_project(project_args(x2, eps2, dir, proj, cu, prompt_len, suffix_len, B, S, d, scratch, scratch_bytes), max_N,
                                    (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_guided_update_packed_project(float* x2, const float* eps2, const float* dir, const float* pcoef, const float* noise,
                                       const int64_t* seeds, uint32_t step, const uint32_t* tags, const float* a, const float* ce,
                                       const float* cz, const int32_t* cu, const int32_t* prompt_len, const int32_t* suffix_len, int B,
                                       int S, int max_N, int d, ditto_stream_t stream) {
    const char* who = "ditto_guided_update_packed_project";
    if (int rc = check_project_ddim(who, pcoef, noise, seeds, a, ce, cz)) return rc;
    if (int rc = check_project_rows(who, x2, eps2, dir, cu, B, S, max_N, d)) return rc;
    HIP_TRY(launch_guided_update_project(x2, eps2, dir, pcoef, noise, seeds, step, tags, a, ce, cz, cu, prompt_len, suffix_len, B, S, max_N,
                                         d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_multistep_update_packed_project(float* x2, const float* eps2, float* q, const float* dir, const float* pcoef,
                                          const ditto_multistep_coef* step, const ditto_multistep_coef* coefs, const int32_t* cu,
                                          const int32_t* prompt_len, const int32_t* suffix_len, int B, int S, int max_N, int d,
                                          ditto_stream_t stream) {
    const char* who = "ditto_multistep_update_packed_project";
    if (int rc = check_project_multistep(who, pcoef, q, step, coefs)) return rc;
    if (int rc = check_project_rows(who, x2, eps2, dir, cu, B, S, max_N, d)) return rc;
    HIP_TRY(launch_multistep_update_project(x2, eps2, q, dir, pcoef, step, coefs, cu, prompt_len, suffix_len, B, S, max_N, d,
                                            (hipStream_t)stream));
    return DITTO_OK;
}

// the forward over [x; x] x [text; null], launch 1 and the finish on its eps, then `update` reading pcoef from the scratch's head
extern "C++" template <class Check, class Update>
static int project_step(PackedStep& p, float* dir, const ditto_project_coef* proj, const int32_t* prompt_len, const int32_t* suffix_len,
                        void* scratch, size_t scratch_bytes, Check&& check, Update&& update) {
    p.forward_over(true);
    return packed_step(p, [&](int d) -> int {
        if (int rc = check_project(p.who, p.x2, p.x2, dir, proj, p.cu_speech, p.B, p.S, p.max_N, d, scratch, scratch_bytes)) return rc;
        return check();
    }, [&](const float* eps, int d) -> int {
        HIP_TRY(launch_guidance_project(project_args(p.x2, eps, dir, proj, p.cu_speech, prompt_len, suffix_len, p.B, p.S, d, scratch,
                                                     scratch_bytes), p.max_N, (hipStream_t)p.stream));
        return update(eps, (const float*)scratch, d);
    });
}

int ditto_guided_step_packed_project_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                          const int32_t* cu_text, const int32_t* prompt_len, const int32_t* suffix_len, float* dir,
                                          const ditto_project_coef* proj, const float* noise, const int64_t* seeds, uint32_t step,
                                          const uint32_t* tags, const float* a, const float* ce, const float* cz, int B, int S, int max_N,
                                          int S_T, int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                          size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                          const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_project_opts");
    return project_step(p, dir, proj, prompt_len, suffix_len, scratch, scratch_bytes, [&]() -> int {
        return check_project_ddim(p.who, (const float*)scratch, noise, seeds, a, ce, cz);
    }, [&](const float* eps, const float* pcoef, int d) -> int {
        HIP_TRY(launch_guided_update_project(x2, eps, dir, pcoef, noise, seeds, step, tags, a, ce, cz, cu_speech, prompt_len, suffix_len, B,
                                             S, max_N, d, (hipStream_t)stream));
        return DITTO_OK;
    });
}

int ditto_guided_step_packed_multistep_project_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t,
                                                    const int32_t* cu_speech, const int32_t* cu_text, const int32_t* prompt_len,
                                                    const int32_t* suffix_len, float* q, float* dir, const ditto_project_coef* proj,
                                                    const ditto_multistep_coef* step, const ditto_multistep_coef* coefs, int B, int S,
                                                    int max_N, int S_T, int max_T, const float* rope_cos, const float* rope_sin,
                                                    void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes,
                                                    ditto_stream_t stream, const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_multistep_project_opts");
    return project_step(p, dir, proj, prompt_len, suffix_len, scratch, scratch_bytes, [&]() -> int {
        return check_project_multistep(p.who, (const float*)scratch, q, step, coefs);
    }, [&](const float* eps, const float* pcoef, int d) -> int {
        HIP_TRY(launch_multistep_update_project(x2, eps, q, dir, pcoef, step, coefs, cu_speech, prompt_len, suffix_len, B, S, max_N, d,
                                                (hipStream_t)stream));
        return DITTO_OK;
    });
}

// ---- projected guidance in a request stream (guided_project_mixed.hip; include/ditto_project_stream.h): a step of projected, plainly
// guided and unguided utterances over the mixed layout; the scratch is project_bytes' ----
// what the three entries share: the rows, the tables, the shapes and the layout
static int check_project_mixed_rows(const char* who, const float* x2, const float* eps2, const float* dir, const int32_t* cu,
                                    const int32_t* partner, const int32_t* kind, int B, int G, int S, int S_G, int max_N, int d) {
    if (!x2 || !eps2 || !dir || !cu || !partner || !kind) return fail(DITTO_ERR_ARG, "%s: null x2 / eps2 / dir / cu / partner / kind", who);
    if (((uintptr_t)x2 | (uintptr_t)eps2 | (uintptr_t)dir) % 16) return fail(DITTO_ERR_ARG, "%s: x2, eps2 and dir must be 16-byte aligned", who);
    if (d <= 0 || d % 64) return fail(DITTO_ERR_SHAPE, "%s: d %% 64 must be 0 (d %d)", who, d);
    if (int rc = check_packed(who, B, S, max_N, S, max_N)) return rc;
    if (!mixed_layout_ok(B, G, S, S_G))
        return fail(DITTO_ERR_SHAPE, "%s: need 0 <= G <= B, G <= S_G <= S, and S_G == 0 exactly when G == 0 (B %d, G %d, S %d, S_G %d)",
                    who, B, G, S, S_G);
    return DITTO_OK;
}
// every argument of launch 1 and the finish
static int check_project_mixed(const char* who, const float* x2, const float* eps2, const float* dir, const ditto_project_coef* proj,
                               const int32_t* cu, const int32_t* partner, const int32_t* kind, int B, int G, int S, int S_G, int max_N,
                               int d, const void* scratch, size_t scratch_bytes) {
    if (!proj || !scratch) return fail(DITTO_ERR_ARG, "%s: null proj / scratch", who);
    if ((uintptr_t)proj % 16) return fail(DITTO_ERR_ARG, "%s: proj must be 16-byte aligned", who);
    if ((uintptr_t)scratch % 256) return fail(DITTO_ERR_ARG, "%s: the project scratch must be 256-byte aligned", who);
    if (int rc = check_project_mixed_rows(who, x2, eps2, dir, cu, partner, kind, B, G, S, S_G, max_N, d)) return rc;
    if (scratch_bytes < project_bytes(B, max_N, d))
        return fail(DITTO_ERR_SIZE, "%s: the project scratch needs %zu bytes (ditto_guidance_project_bytes)", who, project_bytes(B, max_N, d));
    return DITTO_OK;
}
// the update's own: pcoef, the noise and the per-utterance coefficients
static int check_project_mixed_update(const char* who, const float* pcoef, const float* noise, const int64_t* seeds, const uint32_t* tags,
                                      const float* w, const float* a, const float* ce, const float* cz) {
    if (int rc = check_project_ddim(who, pcoef, noise, seeds, a, ce, cz)) return rc;
    if (!w) return fail(DITTO_ERR_ARG, "%s: null w (fp32 [B])", who);
    if (seeds && !tags) return fail(DITTO_ERR_ARG, "%s: seeds need tags (uint32 [B])", who);
    return DITTO_OK;
}
static ProjectMixedArgs project_mixed_args(const float* x2, const float* eps2, float* dir, const ditto_project_coef* proj,
                                           const int32_t* cu, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len,
                                           int B, int G, int S, int S_G, int d, void* scratch, size_t scratch_bytes) {
    ProjectMixedArgs a{};
    a.x2 = x2; a.eps2 = eps2; a.dir = dir; a.proj = proj; a.cu = cu; a.partner = partner; a.kind = kind; a.prompt_len = prompt_len;
    a.B = B; a.G = G; a.S = S; a.S_G = S_G; a.d = d;
    a.pcoef = (float*)scratch;
    a.partial = (double*)((char*)scratch + project_head_bytes(B));
    const size_t slots = (scratch_bytes - project_head_bytes(B)) / ((size_t)B * 4 * sizeof(double));
    a.slots = slots > 0x7fffffff ? 0x7fffffff : (int)slots;
    return a;
}

int ditto_guidance_project_packed_mixed(const float* x2, const float* eps2, float* dir, const ditto_project_coef* proj,
                                        const int32_t* cu, const int32_t* partner, const int32_t* kind, const int32_t* prompt_len, int B,
                                        int G, int S, int S_G, int max_N, int d, void* scratch, size_t scratch_bytes,
                                        ditto_stream_t stream) {
    if (int rc = check_project_mixed("ditto_guidance_project_packed_mixed", x2, eps2, dir, proj, cu, partner, kind, B, G, S, S_G, max_N, d,
                                     scratch, scratch_bytes))
        return rc;
    HIP_TRY(launch_guidance_project_mixed(project_mixed_args(x2, eps2, dir, proj, cu, partner, kind, prompt_len, B, G, S, S_G, d, scratch,
                                                             scratch_bytes), max_N, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_guided_update_packed_project_mixed(float* x2, const float* eps2, const float* dir, const float* pcoef, const float* noise,
                                             const int64_t* seeds, const uint32_t* tags, const float* w, const float* a, const float* ce,
                                             const float* cz, const int32_t* cu, const int32_t* partner, const int32_t* kind,
                                             const int32_t* prompt_len, int B, int G, int S, int S_G, int max_N, int d,
                                             ditto_stream_t stream) {
    const char* who = "ditto_guided_update_packed_project_mixed";
    if (int rc = check_project_mixed_update(who, pcoef, noise, seeds, tags, w, a, ce, cz)) return rc;
    if (int rc = check_project_mixed_rows(who, x2, eps2, dir, cu, partner, kind, B, G, S, S_G, max_N, d)) return rc;
    HIP_TRY(launch_guided_update_project_mixed(x2, eps2, dir, pcoef, noise, seeds, tags, w, a, ce, cz, cu, partner, kind, prompt_len, B, G,
                                               S, S_G, max_N, d, (hipStream_t)stream));
    return DITTO_OK;
}

// the mixed step's forward — over [x; the guided ones' copies] x [text; their null] — then launch 1 and the finish on its eps, then the
// three-kind update reading pcoef from the scratch's head
int ditto_guided_step_packed_project_mixed_opts(ditto_model_t m, float* x2, const void* cond, const int64_t* t, const int32_t* cu_speech,
                                                const int32_t* cu_text, const int32_t* partner, const int32_t* kind,
                                                const int32_t* prompt_len, float* dir, const ditto_project_coef* proj, const float* noise,
                                                const int64_t* seeds, const uint32_t* tags, const float* w, const float* a,
                                                const float* ce, const float* cz, int B, int G, int S, int S_G, int max_N, int S_T,
                                                int max_T, const float* rope_cos, const float* rope_sin, void* workspace,
                                                size_t workspace_bytes, void* scratch, size_t scratch_bytes, ditto_stream_t stream,
                                                const ditto_call_opts* opts) {
    PACKED_STEP(p, "ditto_guided_step_packed_project_mixed_opts");
    return packed_step(p, [&](int d) -> int {
        if (int rc = check_project_mixed(p.who, x2, x2, dir, proj, cu_speech, partner, kind, B, G, S, S_G, max_N, d, scratch, scratch_bytes))
            return rc;
        if (int rc = check_project_mixed_update(p.who, (const float*)scratch, noise, seeds, tags, w, a, ce, cz)) return rc;
        p.nb = B + G; p.rows = S + S_G;   // G <= B and S_G <= S from here on
        return DITTO_OK;
    }, [&](const float* eps, int d) -> int {
        HIP_TRY(launch_guidance_project_mixed(project_mixed_args(x2, eps, dir, proj, cu_speech, partner, kind, prompt_len, B, G, S, S_G, d,
                                                                 scratch, scratch_bytes), max_N, (hipStream_t)stream));
        HIP_TRY(launch_guided_update_project_mixed(x2, eps, dir, (const float*)scratch, noise, seeds, tags, w, a, ce, cz, cu_speech, partner,
                                                   kind, prompt_len, B, G, S, S_G, max_N, d, (hipStream_t)stream));
        return DITTO_OK;
    });
}

int ditto_regroup_packed(const ditto_regroup_seg* table, int n_seg, const void* const* src, const size_t* src_bytes, void* const* dst,
                         const size_t* dst_bytes, int n_bufs, const int64_t* seeds, int n_seeds, size_t max_bytes,
                         ditto_stream_t stream) {
    if (!table || !src || !src_bytes || !dst || !dst_bytes) return fail(DITTO_ERR_ARG, "ditto_regroup_packed: null pointer");
    if (n_seg <= 0 || n_seg > 65535) return fail(DITTO_ERR_SHAPE, "ditto_regroup_packed: n_seg must lie in [1, 65535]");
    if (n_bufs <= 0 || n_bufs > DITTO_REGROUP_BUFS)
        return fail(DITTO_ERR_SHAPE, "ditto_regroup_packed: n_bufs must lie in [1, %d]", DITTO_REGROUP_BUFS);
    if (n_seeds < 0 || (n_seeds > 0 && !seeds)) return fail(DITTO_ERR_ARG, "ditto_regroup_packed: n_seeds without seeds");
    if ((uintptr_t)table % 16) return fail(DITTO_ERR_ARG, "ditto_regroup_packed: the table must be 16-byte aligned");
    RegroupBufs bufs{};
    for (int k = 0; k < n_bufs; ++k) {
        if (((uintptr_t)src[k] | (uintptr_t)dst[k]) % 16)
            return fail(DITTO_ERR_ARG, "ditto_regroup_packed: buffer %d is not 16-byte aligned", k);
        if ((src_bytes[k] >> 36) || (dst_bytes[k] >> 36)) return fail(DITTO_ERR_SIZE, "ditto_regroup_packed: buffer %d exceeds 2^36 bytes", k);
        bufs.src[k] = (const char*)src[k];
        bufs.dst[k] = (char*)dst[k];
        bufs.src_n[k] = src[k] ? (unsigned)(src_bytes[k] / 16) : 0u;
        bufs.dst_n[k] = dst[k] ? (unsigned)(dst_bytes[k] / 16) : 0u;
    }
    HIP_TRY(launch_regroup_packed(table, n_seg, bufs, n_seeds > 0 ? seeds : nullptr, n_seeds, max_bytes / 16, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_regroup_cond_layout(const ditto_config* cfg, int S_T, size_t* kv_row_bytes, size_t* tmod_offset) {
    if (!kv_row_bytes || !tmod_offset) return fail(DITTO_ERR_ARG, "ditto_regroup_cond_layout: null pointer");
    if (int rc = check_cfg(cfg)) return rc;
    if (S_T <= 0) return fail(DITTO_ERR_SHAPE, "ditto_regroup_cond_layout: S_T must be positive");
    *kv_row_bytes = (size_t)cfg->num_layers * 2 * cfg_dp(*cfg) * 2;
    *tmod_offset = al((size_t)S_T * *kv_row_bytes);
    return DITTO_OK;
}

int ditto_quantize_rows_fp8(const float* src, int rows, int cols, void* dst_fp8, float* scales, ditto_stream_t stream) {
    if (!src || !dst_fp8 || !scales || rows <= 0 || cols <= 0) return fail(DITTO_ERR_ARG, "bad argument to ditto_quantize_rows_fp8");
    if (cols % 4) return fail(DITTO_ERR_SHAPE, "cols must be a multiple of 4");
    HIP_TRY(launch_pack_fp8(src, dst_fp8, scales, rows, cols, cols, 1 << 30, 1, 0, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* out_fp8, int M, int d,
                        ditto_stream_t stream) {
    if (!x || !out_fp8 || M <= 0 || d <= 0 || (gamma == nullptr) != (beta == nullptr))
        return fail(DITTO_ERR_ARG, "bad argument to ditto_layernorm_fp8");
    if (d % 4 || d > 2048) return fail(DITTO_ERR_SHAPE, "d must be a multiple of 4 and <= 2048");
    HIP_TRY(launch_layernorm_fp8(x, gamma, beta, out_fp8, d, M, d, (hipStream_t)stream));
    return DITTO_OK;
}

int ditto_gemm_fp8(const void* A, int lda, const void* W, const float* wscale, const float* bias,
                   const float* residual, void* out, int ldo, int M, int N, int K, int epilogue,
                   ditto_stream_t stream) {
    if (!A || !W || !out) return fail(DITTO_ERR_ARG, "null pointer to ditto_gemm_fp8");
    if (K % 128 || N % 16 || lda % 16) return fail(DITTO_ERR_SHAPE, "need K %% 128 == 0, N %% 16 == 0, lda %% 16 == 0");
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.bias = bias; g.residual = residual; g.ldr = ldo; g.out = out; g.ldo = ldo;
    g.M = M; g.N = N; g.K = K; g.fp8 = true; g.wscale = wscale;
    GemmEpilogue e;
    switch (epilogue) {
        case 0: e = EPI_BIAS_BF16; break;
        case 1: e = EPI_BIAS_RES_F32; break;
        case 4: e = EPI_BIAS_F32; break;
        case 5:
            if (!bias || N % 32) return fail(DITTO_ERR_ARG, "gated epilogue needs a bias and N %% 32 == 0");
            e = EPI_GATED_FP8; break;
        default: return fail(DITTO_ERR_ARG, "epilogue must be 0, 1, 4 or 5");
    }
    HIP_TRY(launch_gemm(g, e, (hipStream_t)stream));
    return DITTO_OK;
}

// ditto_gemm_epilogue_bf16's body for the fp8 GEMM: A, W (and the gated output) are bytes, lda / ldw (and the gated ldo) in bytes
int ditto_gemm_epilogue_fp8(const ditto_gemm_epilogue_args* a, const float* wscale, int epilogue, int* structure_out,
                            ditto_stream_t stream) {
    const char* who = "ditto_gemm_epilogue_fp8";
    if (structure_out) *structure_out = 0;
    if (!a || !a->A || !a->W || !a->out) return fail(DITTO_ERR_ARG, "null pointer to %s", who);
    if (epilogue != 0 && epilogue != 1 && epilogue != 2 && epilogue != 4 && epilogue != 5)
        return fail(DITTO_ERR_ARG, "%s: epilogue must be 0, 1, 2, 4 or 5", who);
    const int M = a->M, N = a->N, K = a->K;
    if (M <= 0 || N <= 0 || K <= 0) return fail(DITTO_ERR_SHAPE, "%s: M, N and K must be positive", who);
    if (K % 128 || N % 16) return fail(DITTO_ERR_SHAPE, "%s: need K %% 128 == 0 and N %% 16 == 0", who);
    if (a->lda % 16 || a->lda < K || a->ldw % 16 || (a->ldw && a->ldw < K))
        return fail(DITTO_ERR_SHAPE, "%s: lda / ldw must cover K bytes in multiples of 16 (ldw 0 = K)", who);
    if (a->w_rows < 0 || a->w_rows > N) return fail(DITTO_ERR_SHAPE, "%s: w_rows must be in [0, N] (0 = N)", who);
    const GemmEpilogue e = (GemmEpilogue)epilogue;
    const bool f32_out = e == EPI_BIAS_RES_F32 || e == EPI_BIAS_F32;
    const int out_cols = e == EPI_GATED_FP8 ? N / 2 : N;
    const int ldo_unit = e == EPI_GATED_FP8 ? 8 : (f32_out ? 4 : 8);   // 8-byte pieces of fp8, 16-byte pieces otherwise
    if (a->ldo < out_cols || a->ldo % ldo_unit)
        return fail(DITTO_ERR_SHAPE, "%s: ldo must cover %d columns in multiples of %d", who, out_cols, ldo_unit);
    switch (e) {
        case EPI_BIAS_RES_F32:
            if (a->residual && (a->ldr < N || a->ldr % 4)) return fail(DITTO_ERR_SHAPE, "%s: ldr must cover N columns in multiples of 4", who);
            if (a->out2_bf16 && (a->ldo2 < N || a->ldo2 % 4)) return fail(DITTO_ERR_SHAPE, "%s: ldo2 must cover N columns in multiples of 4", who);
            break;
        case EPI_QKV_ROPE:
            if (!a->rope_cos || !a->rope_sin) return fail(DITTO_ERR_ARG, "%s: the RoPE epilogue needs rope_cos and rope_sin (read unless rope_freq_rev is given)", who);
            if (N % 64 || a->rope_cols % 64 || a->rope_cols < 0 || a->rope_cols > N)
                return fail(DITTO_ERR_SHAPE, "%s: the RoPE epilogue needs N %% 64 == 0 and 0 <= rope_cols <= N in multiples of 64", who);
            if (a->rope_rows_per_batch <= 0) return fail(DITTO_ERR_SHAPE, "%s: epilogue 2 needs rope_rows_per_batch > 0", who);
            break;
        case EPI_GATED_FP8:
            if (!a->bias) return fail(DITTO_ERR_ARG, "%s: the gated epilogue needs a bias", who);
            if (N % 32) return fail(DITTO_ERR_SHAPE, "%s: the gated epilogue needs N %% 32 == 0", who);
            break;
        default: break;
    }
    GemmArgs g{};
    g.A = a->A; g.lda = a->lda; g.W = a->W; g.ldw = a->ldw; g.w_rows = a->w_rows; g.bias = a->bias;
    g.residual = a->residual; g.ldr = a->ldr; g.out = a->out; g.ldo = a->ldo; g.out2_bf16 = a->out2_bf16; g.ldo2 = a->ldo2;
    g.rope_cos = a->rope_cos; g.rope_sin = a->rope_sin; g.rope_rows_per_batch = a->rope_rows_per_batch; g.rope_cols = a->rope_cols;
    g.rope_freq_rev = a->rope_freq_rev;
    g.M = M; g.N = N; g.K = K; g.fp8 = true; g.wscale = wscale;
    const hipError_t err = launch_gemm(g, e, (hipStream_t)stream);
    if (structure_out) *structure_out = t_gemm_structure;
    HIP_TRY(err);
    return DITTO_OK;
}

// plain integer switches: one slot each (ditto_get_option reads them; ditto_set_option validates per name below)
static int* option_slot(const char* name) {
    static const struct { const char* n; int* p; } tab[] = {
        {"gemm_tile", &g_gemm_tile}, {"attn_flags", &g_attn_flags}, {"gemm_flags", &g_gemm_flags}, {"gemm_group", &g_gemm_group},
        {"pp_mask", &g_pp_mask}, {"fr_mask", &g_fr_mask}, {"fr_class_rows", &g_fr_class_rows}, {"fr_dgrad", &g_fr_dgrad},
        {"train_flags", &g_train_flags}, {"fr_u_fp8", &g_fr_u_fp8}, {"fr_hb", &g_fr_hb}, {"fr_tile", &g_fr_tile}, {"fr64_maxk", &g_fr64_maxk},
        {"fr_stagger", &g_fr_stagger}, {"fr_rot", &g_fr_rot}, {"pp_nb", &g_pp_nb}, {"pp_stagger", &g_pp_stagger},
        {"splitk_wgs", &g_splitk_wgs}, {"residual_bf16", &g_resid_bf16}, {"lnq", &g_lnq}, {"lnq_ring", &g_lnq_ring}, {"lnq_waves", &g_lnq_waves}, {"qkv_split", &g_qkv_split}, {"ll_mask", &g_ll_mask}, {"lnq_min_rows", &g_lnq_min_rows}, {"attn64p_min_wgs", &g_attn64p_min_wgs}, {"attn64p_min_wgs_plain", &g_attn64p_min_wgs_plain},
        {"slp_lr_chunk", &g_slp_lr_chunk}, {"slp_last_row", &g_slp_last_row}, {"attn_generic_kib", &g_attn_generic_kib}};
    for (auto& e : tab) if (!strcmp(name, e.n)) return e.p;
    return nullptr;
}

int ditto_get_option(const char* name, int* value) {
    if (!name || !value) return fail(DITTO_ERR_ARG, "null argument to ditto_get_option");
    if (!strcmp(name, "wgrad_wgs")) { *value = get_wgrad_wgs(); return DITTO_OK; }
    if (const int* p = option_slot(name)) { *value = *p; return DITTO_OK; }
    return fail(DITTO_ERR_ARG, "unknown option '%s'", name);
}

int ditto_set_option(const char* name, int value) {
    if (!name) return fail(DITTO_ERR_ARG, "null option name");
    if (!strcmp(name, "gemm_tile")) {
        if (value != 0 && value != 127 && value != 128 && value != 256 && value != 129 && value != 131 && value != 192)
            return fail(DITTO_ERR_ARG, "gemm_tile must be 0, 127 (128x128 deep prefetch), 128, 129 (256x128 ring), "
                                       "131 (128x256 ping-pong, 2 workgroups/CU), 192 (256x192 where the epilogue allows) or 256");
        g_gemm_tile = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "slp_lr_chunk")) {   // keys per workgroup of the last-row attention kernel (attention_slp.hip)
        if (value < 1 || value > 1024) return fail(DITTO_ERR_ARG, "slp_lr_chunk must be in [1, 1024]");
        g_slp_lr_chunk = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "slp_last_row")) {   // ditto_slp_forward_varlen: 1 = last layer on the last rows only, 0 = composed (A/B)
        if (value != 0 && value != 1) return fail(DITTO_ERR_ARG, "slp_last_row must be 0 or 1");
        g_slp_last_row = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "attn_generic_kib")) {   // test hook: scratch budget of the GEMM-composed attention, KiB (attention.hip generic_chunk)
        if (value < 1) return fail(DITTO_ERR_ARG, "attn_generic_kib must be >= 1 (default 2097152 = 2 GiB)");
        g_attn_generic_kib = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "attn_flags")) {
        g_attn_flags = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "wgrad_wgs")) {
        if (value < 0 || value > 2048) return fail(DITTO_ERR_ARG, "wgrad_wgs must be in [0, 2048] (0 = cost model)");
        set_wgrad_wgs(value);
        return DITTO_OK;
    }
    if (!strcmp(name, "gemm_flags")) {
        g_gemm_flags = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "gemm_group")) {
        if (value < 0 || value > 64) return fail(DITTO_ERR_ARG, "gemm_group must be in [0, 64]");
        g_gemm_group = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "pp_mask")) {
        if (value < -1 || value > 63) return fail(DITTO_ERR_ARG, "pp_mask must be in [-1, 63]");
        g_pp_mask = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_mask")) {
        if (value < 0 || value > 3) return fail(DITTO_ERR_ARG, "fr_mask must be in [0, 3]");
        g_fr_mask = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_class_rows")) {
        if (value < 0) return fail(DITTO_ERR_ARG, "fr_class_rows must be >= 0 (0 = every launch decides on its own rows)");
        g_fr_class_rows = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_dgrad")) {
        if (value < 0 || value > 3) return fail(DITTO_ERR_ARG, "fr_dgrad must be in [0, 3]");
        g_fr_dgrad = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "train_flags")) {
        if (value < 0 || value > 31) return fail(DITTO_ERR_ARG, "train_flags must be in [0, 31]");
        g_train_flags = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_u_fp8")) {   // test hook: ditto_gemm_ln_bf16 writes u as fp8 e4m3 bytes ([M, ldu] bytes; N = 1024)
        g_fr_u_fp8 = value != 0;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_hb")) {   // test hook: ditto_gemm_ln_bf16's residual and out are bf16 [M, ldo] (the bf16 residual stream's kernel form; N = 768)
        g_fr_hb = value != 0;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_tile")) {
        if (value != 0 && value != 64 && value != 130) return fail(DITTO_ERR_ARG, "fr_tile must be 0 (rule), 64 or 130 (128 rows, W straight into registers)");
        g_fr_tile = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr64_maxk")) {
        if (value < 0) return fail(DITTO_ERR_ARG, "fr64_maxk must be >= 0");
        g_fr64_maxk = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_stagger")) {
        if (value < 0 || value > 100000) return fail(DITTO_ERR_ARG, "fr_stagger must be in [0, 100000] (10 ns ticks)");
        g_fr_stagger = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "fr_rot")) {
        if (value < 0 || value > 4096) return fail(DITTO_ERR_ARG, "fr_rot must be in [0, 4096]");
        g_fr_rot = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "pp_nb")) {
        if (value != 0 && value != 3 && value != 4) return fail(DITTO_ERR_ARG, "pp_nb must be 0 (rule), 3 (192-wide tiles) or 4 (256-wide)");
        g_pp_nb = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "pp_stagger")) {
        if (value < -1 || value > 100000) return fail(DITTO_ERR_ARG, "pp_stagger must be in [-1, 100000] (10 ns ticks; -1 = rule)");
        g_pp_stagger = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "lnq_min_rows")) {
        if (value < 0) return fail(DITTO_ERR_ARG, "lnq_min_rows must be >= 0");
        g_lnq_min_rows = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "attn64p_min_wgs") || !strcmp(name, "attn64p_min_wgs_plain")) {
        if (value < 1) return fail(DITTO_ERR_ARG, "attn64p_min_wgs[_plain] must be >= 1");
        (name[15] ? g_attn64p_min_wgs_plain : g_attn64p_min_wgs) = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "ll_mask")) {
        if (value < 0 || value > 3) return fail(DITTO_ERR_ARG, "ll_mask must be in [0, 3]");
        g_ll_mask = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "lnq_waves")) {
        if (value != 4 && value != 8) return fail(DITTO_ERR_ARG, "lnq_waves must be 4 (one wave per SIMD) or 8 (two)");
        g_lnq_waves = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "qkv_split")) {
        if (value < 0 || value > 64) return fail(DITTO_ERR_ARG, "qkv_split must be in [0, 64]");
        g_qkv_split = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "lnq_ring")) {
        if (value != 0 && value != 2 && value != 4 && value != 8) return fail(DITTO_ERR_ARG, "lnq_ring must be 0 (default), 4 or 8 (shape 32), 2 or 4 (shape 16)");
        g_lnq_ring = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "lnq")) {
        if (value != 0 && value != 16 && value != 32) return fail(DITTO_ERR_ARG, "lnq must be 0 (off), 32 or 16 (MFMA shape)");
        g_lnq = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "residual_bf16")) {
        if (value < 0 || value > 1) return fail(DITTO_ERR_ARG, "residual_bf16 must be 0 or 1");
        g_resid_bf16 = value;
        return DITTO_OK;
    }
    if (!strcmp(name, "splitk_wgs")) {
        if (value < -1 || value > 2048) return fail(DITTO_ERR_ARG, "splitk_wgs must be in [-1, 2048] (-1 never, 0 the low-latency class rule, > 0 a workgroup target)");
        g_splitk_wgs = value;
        return DITTO_OK;
    }
    return fail(DITTO_ERR_ARG, "unknown option '%s'", name);
}

int ditto_full_row_plan(const ditto_config* cfg, int B, int N, int* outproj, int* fc2) {
    return ditto_full_row_plan_opts(cfg, B, N, nullptr, outproj, fc2, nullptr);
}

int ditto_full_row_plan_opts(const ditto_config* cfg, int B, int N, const ditto_call_opts* opts, int* outproj, int* fc2,
                             int* stream_bf16) {
    return with_opts(opts, [&]() -> int {
        if (int rc = check_cfg(cfg)) return rc;
        if (!outproj || !fc2 || B <= 0 || N <= 0) return fail(DITTO_ERR_ARG, "bad argument to ditto_full_row_plan");
        if ((long long)B * N > 0x7fffffffLL) return fail(DITTO_ERR_SHAPE, "B * N exceeds 2^31 - 1 rows");
        ForwardPlan fp;   // the forward's own plan (the scratch-dependent K-splits are not part of the answer)
        if (int rc = plan_forward(*cfg, B * N, 0, PLAN_QUERY, &fp)) return rc;
        *outproj = fp.fr_out; *fc2 = fp.fr_fc2;
        if (stream_bf16) *stream_bf16 = fp.hb;
        return DITTO_OK;
    });
}

int ditto_profile_enable(ditto_model_t m, int enable) {
    if (!m) return fail(DITTO_ERR_ARG, "null model");
    m->prof = enable != 0;
    return DITTO_OK;
}

int ditto_profile_read(ditto_model_t m, int32_t* launches, float* ms) {
    if (!m || !launches || !ms) return fail(DITTO_ERR_ARG, "null argument to ditto_profile_read");
    for (auto& r : m->recs) {
        HIP_TRY(hipEventSynchronize(r.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        m->launches[r.kc] += 1;
        m->ms[r.kc] += t;
        m->pool.push_back(r.a);
        m->pool.push_back(r.b);
    }
    m->recs.clear();
    for (int i = 0; i < DITTO_KC_COUNT; ++i) {
        launches[i] = m->launches[i]; ms[i] = m->ms[i];
        m->launches[i] = 0; m->ms[i] = 0.f;
    }
    return DITTO_OK;
}

}  // extern "C"
