// batch_layout.h — internal: which of the three layouts a batch is in and what the layout-aware launches read from it.
//   dense   B utterances of exactly N speech and T text rows: x [B, N, d], the conditioning's K / V rows [B, T, .]
//   padded  the same buffers, utterance b valid on its first speech_len[b] / text_len[b] rows only
//   packed  utterances concatenated along the rows: utterance b owns speech rows [cu[b], cu[b+1]) of the M rows and text rows
//           [cu_t[b], cu_t[b+1]) of the Mt rows; N / T are then the longest utterance's
// Row-wise launches take M (or Mt) alone; the attention, the AdaLN entry, the QKV epilogue, the padded rows' zeroing ask for more.
#pragma once
#include "model.h"

namespace ditto {

struct __attribute__((visibility("hidden"))) BatchLayout {   // hidden: the library exports nothing of it
    enum Kind { DENSE, PADDED, PACKED } kind;
    int B;                                  // utterances
    int M, Mt;                              // rows of the speech side (x, h, eps) and of the text side (K / V of the conditioning)
    int N, T;                               // speech / text rows per utterance: the stride (dense, padded) or the longest (packed)
    const int32_t *speech_len, *text_len;   // padded: device int32 [B]
    const int32_t *cu, *cu_t;               // packed: device int32 [B + 1]

    static BatchLayout padded(int B, int N, int T, const int32_t* speech_len, const int32_t* text_len) {   // no lengths: dense
        return {speech_len || text_len ? PADDED : DENSE, B, B * N, B * T, N, T, speech_len, text_len, nullptr, nullptr};
    }
    static BatchLayout dense(int B, int N, int T) { return padded(B, N, T, nullptr, nullptr); }
    static BatchLayout packed(int B, int S, int max_N, int S_T, int max_T, const int32_t* cu, const int32_t* cu_t) {
        return {PACKED, B, S, S_T, max_N, max_T, nullptr, nullptr, cu, cu_t};
    }

    bool varlen() const { return kind != DENSE; }
    // K-loop rotation period of the full-row GEMMs / gemm_lnq in their `tile`-row tiles, 0 = unrotated.  Dense only: it is a function
    // of the padded N, and an utterance's bits must not depend on the padding (a packed batch's tiles straddle utterances anyway)
    int rot_period(int tile) const { return kind == DENSE && N % tile == 0 ? N / tile : 0; }
    // the RoPE position of row r in the QKV epilogue: r % this; a packed batch reads it from the row map instead (Ws::pos)
    int rope_rows_per_batch() const { return kind == PACKED ? M : N; }
    // self-attention (speech x speech) or cross-attention (speech x text): batch, extents and per-utterance bounds
    void fill_attn(AttnArgs& a, bool cross) const {
        a.B = B; a.Sq = N; a.Skv = cross ? T : N;
        if (kind == PADDED) { a.q_len = speech_len; a.kv_len = cross ? text_len : speech_len; }
        if (kind == PACKED) { a.cu_q = cu; a.cu_kv = cross ? cu_t : cu; a.q_rows = M; a.kv_rows = cross ? Mt : M; }
    }
    // cond = K / V rows of every layer [Mt, L * 2 dp] bf16 | tmod fp32 [B, 2d]
    size_t tmod_offset(const ditto_config& c) const { return al((size_t)Mt * c.num_layers * 2 * cfg_dp(c) * 2); }
    // the workspace plan of a forward over this batch (ditto_api.hip: plan_ws, or the packed plan with its two row maps)
    WsPlan plan(const ditto_config& c) const;
};

}  // namespace ditto
