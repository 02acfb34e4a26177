"""The fused attention's fp64 reference and an elementwise error bound derived from the kernels' arithmetic (plain helpers,
shared by test_attention_bound.py, test_gpu_attention_resid.py and test_gpu_kernels.py; for the GEMM-composed path with its masks
and lengths, at the end: test_attention_composed_bound.py and test_gpu_attention_composed_elementwise.py).

Every kernel computes, per (batch, head, query row), scores s_j = q.k_j in fp32 (log2 units: q pre-scaled by scale * log2(e), or
the fp32 product times scale * log2(e)), probabilities p_j = exp2(s_j - c) for some shift c, rounds each p_j to bf16 (relative
error <= u = 2^-8) before the P V product, and divides by a row sum l that is the fp32 sum of the p_j or of their bf16 roundings.
The output is therefore a convex combination of the V rows whose weights w_j are perturbed by at most 2u (plus fp32 sums):

    |o - o_ref| <= A * sum_j w_j |v[j, col]|,  A = 2u + 2 gamma(Skv) + 2 ln2 gamma(dh) * max_j sum_i |q_i k_ji| + fp32 slack

(gamma(n) = n 2^-24, the fp32 sums of the row sum, of the P V accumulation and of the score dot products).  sum_j w_j |v[j, col]|
<= max_j |v[j, col]|, so this is at least as tight as the 2^-7 max_j |v| form.  A result stored as bf16 adds half an ulp of itself
(at most 2^-8 of it, granted by worst_ratio); the residual add and the 1 / l scaling add a few fp32 roundings.  None of this depends on the data being benign, so a kernel that is
right passes it on every element, and one that gets a score block, a key tile, the mask or the residual wrong fails it on some
element once the data make a few keys matter (sharp softmax rows: make_case)."""
import math

import torch

from gpu_util import asym

LOG2E = 1.4426950408889634
U = 2.0 ** -8     # bf16 unit roundoff (round to nearest even, 8 significant bits)
G = 2.0 ** -24    # fp32's


def make_case(B, H, Sq, Skv, seed, dh=64, sharp=2.5, late=True, device="cpu"):
    """q (pre-scaled by scale * log2(e), rounded to bf16), k, v (bf16) [rows, H * dh] and scale.  Natural-log logits of std `sharp`:
    a few keys carry most of a row's weight, so a wrong tile or block moves the output by O(|v|).  `late`: two rows of every
    (batch, head) get one key far above the rest (+40 / +30 log2 units), in the last tile and in tile 1: raises of the running
    maximum late in the loop on the kernels that keep one."""
    scale = 1.0 / math.sqrt(dh)
    q = asym((B * Sq, H * dh), seed) * sharp
    k = asym((B * Skv, H * dh), seed + 1)
    v = asym((B * Skv, H * dh), seed + 2)
    if late and Skv > 70 and Sq > 9:
        for b in range(B):
            for h in range(H):
                cols = slice(h * dh, (h + 1) * dh)
                for row, key, lg2 in ((5, Skv - 3, 40.0), (9, 70, 30.0)):
                    qr = q[b * Sq + row, cols]
                    k[b * Skv + key, cols] = qr * (lg2 / (LOG2E * scale * float(qr @ qr)))
    qs = (q * (LOG2E * scale)).to(torch.bfloat16)
    return qs.to(device), k.to(torch.bfloat16).to(device), v.to(torch.bfloat16).to(device), scale


def _heads(x, b, h, rows, dh):
    return x[b * rows:(b + 1) * rows, h * dh:(h + 1) * dh]


def reference(q, k, v, B, H, Sq, Skv, dh, log2_scale=1.0, vis=None):
    """fp64 on the exact operands: o [B*Sq, H*dh], wabs = sum_j w_j |v[j, col]| (same shape), s1 [B*Sq, H] = max_j sum_i |q_i k_ji|
    in log2 units.  log2_scale: 1 for pre-scaled q, scale * log2(e) otherwise.  vis (integer [B, Sq], see visible_keys): row i of
    batch b attends to keys 0 .. vis[b, i] - 1 only and nothing else of k / v enters its result (NaN there is legal); a row that
    sees no key has o = wabs = s1 = 0, so its bound is the floor and only an exact 0 passes.  None: every key."""
    dev = q.device
    o = torch.empty(B * Sq, H * dh, dtype=torch.float64, device=dev)
    wabs = torch.empty_like(o)
    s1 = torch.empty(B * Sq, H, dtype=torch.float64, device=dev)
    for b in range(B):
        for h in range(H):
            Q, K, V = (_heads(x, b, h, n, dh).double() for x, n in ((q, Sq), (k, Skv), (v, Skv)))
            if vis is not None:
                n = vis[b].to(dev)
                seen = torch.arange(Skv, device=dev)[None, :] < n[:, None]                 # [Sq, Skv]
                used = (torch.arange(Skv, device=dev) < n.max())[:, None]                  # keys some row sees
                Q, K, V = torch.where((n > 0)[:, None], Q, 0.0), torch.where(used, K, 0.0), torch.where(used, V, 0.0)
                S = torch.where(seen, (Q @ K.T) * log2_scale, -math.inf)
                m = S.amax(1, keepdim=True)
                P = torch.exp2(S - torch.where(torch.isfinite(m), m, 0.0))                 # masked keys: exactly 0
                W = P / P.sum(1, keepdim=True).clamp_min(1e-300)
                _heads(o, b, h, Sq, dh)[:] = W @ V
                _heads(wabs, b, h, Sq, dh)[:] = W @ V.abs()
                s1[b * Sq:(b + 1) * Sq, h] = torch.where(seen, Q.abs() @ K.abs().T, 0.0).amax(1) * abs(log2_scale)
                continue
            S = (Q @ K.T) * log2_scale
            P = torch.exp2(S - S.amax(1, keepdim=True))
            W = P / P.sum(1, keepdim=True)
            _heads(o, b, h, Sq, dh)[:] = W @ V
            _heads(wabs, b, h, Sq, dh)[:] = W @ V.abs()
            s1[b * Sq:(b + 1) * Sq, h] = (Q.abs() @ K.abs().T).amax(1) * abs(log2_scale)
    return o, wabs, s1


def bound(o, wabs, s1, Skv, dh, resid=None):
    """want = o (+ resid) and the elementwise bound on |got - want| before any bf16 store: see the module docstring."""
    H = s1.shape[1]
    A = 2 * U + (2 * Skv + 256) * G + 2 * math.log(2) * (dh + 8) * G * s1.repeat_interleave(o.shape[1] // H, dim=1)
    want = o if resid is None else o + resid.double()
    return want, A * wabs + 8 * G * o.abs() + 2 * G * want.abs() + 1e-30


def worst_ratio(got, want, e, stored_bf16=False):
    """max |got - want| / e over every element (inf where got is not finite, 0 for no element).  stored_bf16: got is the bf16 rounding
    of a value within e of want, so half a bf16 ulp of got is granted on top of e (the ratio is that of the arithmetic before it)."""
    if got.numel() == 0:
        return 0.0
    g = got.double()
    d = (g - want).abs()
    if stored_bf16:
        _, ex = torch.frexp(g)
        d = (d - torch.ldexp(torch.ones_like(g), ex - 9)).clamp_min(0.0)    # |g| in [2^(ex-1), 2^ex): half an ulp is 2^(ex-9)
    d = d / e
    d = torch.where(torch.isfinite(g), d, torch.full_like(d, math.inf))
    return float(d.max())


def emulate(q, k, v, B, H, Sq, Skv, dh, rowsum_bf16=False, mutate=None, tile=None):
    """A CPU model of the kernels' arithmetic (pre-scaled q): fp32 scores, P = exp2(s - rowmax) rounded to bf16, row sum of the fp32
    (attn64p / attn64q) or of the rounded (attn64v2 / v3) probabilities, fp32 P V — and the bugs the bound must catch:
      "stale_block": the 32-key score block 1 of key tile `tile` taken from tile - 1 (a stale accumulator), query rows 0..31 of each 64;
      "drop_num" / "drop_sum": key tile `tile` left out of the numerator / of the row sum;
      "unmasked": the partial last tile's missing key rows counted, as the clamped copies of key Skv - 1 the kernels load there."""
    o = torch.empty(B * Sq, H * dh, dtype=torch.float32)
    for b in range(B):
        for h in range(H):
            Q, K, V = (_heads(x, b, h, n, dh).float() for x, n in ((q, Sq), (k, Skv), (v, Skv)))
            if mutate == "unmasked":
                pad = (-Skv) % 64
                assert pad, "unmasked needs a partial last tile"
                K = torch.cat([K, K[-1:].expand(pad, dh)])
                V = torch.cat([V, V[-1:].expand(pad, dh)])
            S = Q @ K.T
            if mutate == "stale_block":
                a = tile * 64 + 32
                rows = (torch.arange(Sq) % 64) < 32
                S[rows, a:a + 32] = S[rows, a - 64:a - 32]
            P = torch.exp2(S - S.amax(1, keepdim=True)).to(torch.bfloat16).float()
            keep = torch.ones(K.shape[0], dtype=torch.bool)
            if mutate in ("drop_num", "drop_sum"):
                keep[tile * 64:(tile + 1) * 64] = False
            Pl = P if rowsum_bf16 else torch.exp2(S - S.amax(1, keepdim=True))
            ls = (Pl * keep).sum(1, keepdim=True) if mutate == "drop_sum" else Pl.sum(1, keepdim=True)
            num = (P * keep) @ V if mutate == "drop_num" else P @ V
            _heads(o, b, h, Sq, dh)[:] = num / ls
    return o


# ---- the GEMM-composed path (any head_dim that is not 64; csrc/attention.hip "generic head_dim", csrc/attention_slp.hip) ----
def _lens(lens, B, full):
    """per-utterance lengths as the kernels read them: None = full, values clamped to [1, full]"""
    return [full] * B if lens is None else [min(max(int(n), 1), full) for n in lens]


def visible_keys(B, Sq, Skv, q_len=None, kv_len=None, causal=False, padded_offset=False):
    """int64 [B, Sq]: how many keys row i of utterance b sees, by the kernels' rule: clamp(i + (kl - ql) + 1, 0, kl) if causal,
    else kl, and 0 for i >= ql.  The dense causal entry is ql = Sq, kl = Skv.  padded_offset: the BUG of taking the padded
    batch's causal offset Skv - Sq for the utterance's own kl - ql."""
    ql, kl = torch.tensor(_lens(q_len, B, Sq))[:, None], torch.tensor(_lens(kv_len, B, Skv))[:, None]
    i = torch.arange(Sq)[None, :]
    n = kl.expand(B, Sq)
    if causal:
        off = torch.full_like(kl, Skv - Sq) if padded_offset else kl - ql
        n = torch.minimum((i + off + 1).clamp_min(0), kl)
    return torch.where(i < ql, n, torch.zeros_like(n)).contiguous()


def make_masked_case(B, H, Sq, Skv, dh, seed, q_len=None, kv_len=None, causal=False, device="cpu"):
    """q [B*Sq, H*dh], k, v [B*Skv, H*dh] (bf16, q NOT pre-scaled) and scale = 1 / sqrt(dh): sharp rows on both sides of every mask
    edge.  An ALIGNED key j is a multiple of some query row, with natural-log logit ln(j + 1) + 6 after the scale: about e^6 times
    the mass of each other key (logits of unit variance), so it carries that row; its value row is +-2.5 + noise, the others' are
    noise, so losing or gaining it moves the row by O(|v|).
      causal, off = kl - ql, every key j of the buffer, r = j - off:
        r % 3 == 0: aligned with query r     — the diagonal, that row's LAST visible key;
        r % 3 == 2: aligned with query r - 1 — that row's FIRST masked key (for the last row, key kl: in the padding);
      not causal: key kl - 1 aligned with the last valid query row, key kl (the first padded one, if the buffer has it) with the
      middle one.
    Rows at or past the lengths hold finite data here; a test that wants NaN there overwrites them."""
    D, scale = H * dh, 1.0 / math.sqrt(dh)
    q, k = asym((B, Sq, D), seed), asym((B, Skv, D), seed + 1)
    vv = asym((B, Skv, D), seed + 2)
    v = vv.clone()
    qls, kls = _lens(q_len, B, Sq), _lens(kv_len, B, Skv)
    for b in range(B):
        ql, kl = qls[b], kls[b]
        pairs = []                                          # (key, query row it is aligned with)
        if causal:
            off = kl - ql
            for j in range(Skv):
                r = j - off
                if r % 3 == 0 and 0 <= r < ql:
                    pairs.append((j, r))
                elif r % 3 == 2 and 0 <= r - 1 < ql:
                    pairs.append((j, r - 1))
        else:
            pairs.append((kl - 1, ql - 1))
            if kl < Skv:
                pairs.append((kl, (ql - 1) // 2))
        for j, r in pairs:
            for h in range(H):
                c = slice(h * dh, (h + 1) * dh)
                qr = q[b, r, c]
                k[b, j, c] = qr * ((math.log(j + 1) + 6.0) / (scale * float(qr @ qr)))
                v[b, j, c] = (2.5 if (b + h + j // 3) % 2 == 0 else -2.5) + 0.5 * vv[b, j, c]
    q, k, v = (t.reshape(-1, D).to(torch.bfloat16).to(device) for t in (q, k, v))
    return q, k, v, scale


def emulate_composed(q, k, v, B, H, Sq, Skv, dh, scale, q_len=None, kv_len=None, causal=False, mutate=None):
    """A CPU model of the composed path's arithmetic: fp32 scores, p = exp2((s - rowmax) * scale * log2(e)) over the visible keys,
    times 1 / sum, rounded to bf16, fp32 P V (V rows no row sees count as zeros); fp32 [B*Sq, H*dh].  And the bugs the bound must
    catch:
      "one_fewer" / "one_more": every valid row sees one key fewer / one more (while the buffer has one: it may be a padded row);
      "padded_offset": the causal offset Skv - Sq of the padded batch instead of the utterance's kl - ql;
      "wrong_head": head h multiplies the V of head (h + 1) % H — a wrong head offset or stride in a chunk of (batch, head) pairs."""
    assert mutate in (None, "one_fewer", "one_more", "padded_offset", "wrong_head")
    vis = visible_keys(B, Sq, Skv, q_len, kv_len, causal, padded_offset=mutate == "padded_offset")
    valid = torch.arange(Sq)[None, :] < torch.tensor(_lens(q_len, B, Sq))[:, None]
    if mutate == "one_fewer":
        vis = (vis - 1).clamp_min(0)
    if mutate == "one_more":
        vis = torch.where(valid, (vis + 1).clamp_max(Skv), vis)
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    o = torch.zeros(B * Sq, H * dh, dtype=torch.float32)
    for b in range(B):
        seen = torch.arange(Skv)[None, :] < vis[b][:, None]
        used = (torch.arange(Skv) < vis[b].max())[:, None]
        for h in range(H):
            hv = (h + 1) % H if mutate == "wrong_head" else h
            Q, K = _heads(q, b, h, Sq, dh).float(), _heads(k, b, h, Skv, dh).float()
            V = torch.where(used, _heads(v, b, hv, Skv, dh).float(), 0.0)
            S = torch.where(seen, torch.where(used.T, Q @ K.T, 0.0), -math.inf)
            m = S.amax(1, keepdim=True)
            P = torch.exp2((S - torch.where(torch.isfinite(m), m, 0.0)) * sl2)
            s = P.sum(1, keepdim=True)
            P = (P * torch.where(s > 0, 1.0 / s, 0.0)).to(torch.bfloat16).float()
            _heads(o, b, h, Sq, dh)[:] = torch.where((vis[b] > 0)[:, None], P @ V, 0.0)
    return o
