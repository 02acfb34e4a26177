"""The fused attention's fp64 reference and an elementwise error bound derived from the kernels' arithmetic (plain helpers,
shared by test_attention_bound.py, test_gpu_attention_resid.py and test_gpu_kernels.py).

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


def reference(q, k, v, B, H, Sq, Skv, dh, log2_scale=1.0):
    """fp64 on the exact operands: o [B*Sq, H*dh], wabs = sum_j w_j |v[j, col]| (same shape), s1 [B*Sq, H] = max_j sum_i |q_i k_ji|
    in log2 units.  log2_scale: 1 for pre-scaled q, scale * log2(e) otherwise."""
    dev = q.device
    o = torch.empty(B * Sq, H * dh, dtype=torch.float64, device=dev)
    wabs = torch.empty_like(o)
    s1 = torch.empty(B * Sq, H, dtype=torch.float64, device=dev)
    for b in range(B):
        for h in range(H):
            Q, K, V = (_heads(x, b, h, n, dh).double() for x, n in ((q, Sq), (k, Skv), (v, Skv)))
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
