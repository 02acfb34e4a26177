"""fp64 references, elementwise error bounds, test data and fp32 emulations for the forward row kernels of csrc/rowwise.hip: ln_kernel in
its AdaLN modes (dense and packed), splitk_finish_kernel / splitk_finish_ln_kernel, text_pool_kernel / text_pool_packed_kernel /
text_mod_kernel, time_table_kernel, packed_row_map_kernel and rope_table_kernel.  Shared by test_rowwise_ref.py (no GPU: the references
against torch, the fp32 emulation inside every bound, every mutant of a wrong kernel outside one) and test_gpu_rowwise.py (the kernels).
Every function returns the expected value AND a bound on |kernel - expected|; a bound is computed from the inputs and the fp64 reference,
never from the kernel's output.  G = u = 2^-24 below; layernorm_terms / layernorm / row_factors / worst_ratio are gemm_fp8_ref's, so the
LayerNorm statistics have one derivation in the suite (mean em = (d + 1) u mean|x|, variance ev, rstd er: gemm_fp8_ref.py).

* AdaLN h (`adaln_ref`): t = (x - mean) rstd, scale = 1 + sc_t + sc_x, shift = sh_t + sh_x, h = t scale + shift (reference
  src/components/DiT.py:34-39).  The kernel's t32 is within  et = em rstd + |t| (er + 2 u)  of t (the statistics, the subtraction, the
  multiplication by rstd).  scale32 = fl(fl(1 + sc_t) + sc_x): two roundings, es = u (|1 + sc_t| + |scale|).  shift32: one, u |shift|.
  h32 = t32 scale32 + shift32 is one fma or a product and a sum (the compiler may contract): u |t scale| + u |h| covers both.  So
      |h32 - h| <= |scale| et + |t| es + u |t scale| + u |shift| + u |h|,
  then, for the bf16 stream, half a bf16 ulp of the stored value (worst_ratio(stored="bf16")).  The raw copy is bf16(x) bit for bit.
  Through ditto_global_adaln the two tables are themselves kernel outputs (two text-modulation launches, bounds e_tt, e_tm below): the
  kernel's scale and shift move by at most e_sc = e_tt + e_tm of each half, so (|t| + et) e_sc + e_sh is added (`adaln_ref(e_ttab=...)`).
* u1 (`u1_ref`): with an fp32 h the kernel normalises the values it stores, so the reference is the fp64 LayerNorm of the kernel's own h
  output (pinned elementwise by the h assertion) with gemm_fp8_ref.layernorm's bound (ln_norm is the same explicit fma), then the bf16
  store grant; the GPU test also holds it bitwise to ditto_layernorm_bf16 on that h.  With a bf16 h the kernel normalises the UNROUNDED
  fp32 row, of which only the bf16 rounding is visible: the reference is LayerNorm64 of the fp64 h and the h bound is propagated through
  the statistics (gemm_fr_ref.layernorm_of_perturbed: derived there).
* split-K finish (`finish_chain`, `finish_ref`): out = ((p_0 + p_1 + ... + p_{n-1}) + bias) + residual, every + one fp32 addition in that
  order: no product, nothing to contract, so `finish_chain` (the same additions in torch fp32 on the CPU) is the kernel's out BIT FOR BIT,
  and out2 is bitwise its bf16 rounding.  Against fp64: at most nsplit + 1 additions, each rounding a partial sum <= S = sum |p_s| + |bias|
  + |residual|:  |out32 - out64| <= (nsplit + 2) u S  (one spare, as acc_bound).  u = LayerNorm(out): the fp64 LayerNorm of the fp32
  chain with gemm_fp8_ref.layernorm's bound and the bf16 grant; bitwise the two-launch form on the GPU.
* text pool (`pool_ref`): T_b - 1 fp32 additions in four row groups and a division: |p32 - p| <= (T_b + 1) u mean_T|x|.
* text modulation (`text_mod_ref`): s = silu(p), tmod = W s + b.  silu32 is within  es = 1.1 ep + SILU_MULT f |s|  of s: |silu'| <= 1.0998
  propagates the pool's ep, f is the measured floor (below).  Each lane adds ceil(dt / 64) fmas, the wave sum 6 additions, the bias one:
  at most dt + 1 roundings of partial sums <= |W| |s32| + |b|:   |tmod32 - tmod| <= |W| es + (dt + 2) u (|W| (|s| + es) + |b|).
* time table (`time_table_ref`): z1 = W0 e + b0, a = silu(z1), z2 = W2 a + b2, c = silu(z2), out = Wt c + bt.  Each dot product is a
  chain of td fmas and an addition, (td + 1) u (|W| |v| + |b|) (acc_bound at td), and each stage propagates its input's bound:
  e_z1 = acc_bound;  e_a = 1.1 e_z1 + SILU_MULT f |a|;  e_z2 = |W2| e_a + acc_bound(|W2| (|a| + e_a) + |b2|);  e_c likewise;
  e_out = |Wt| e_c + acc_bound(|Wt| (|c| + e_c) + |bt|).
* packed row map (`row_map_ref`): numpy.searchsorted(cu[:B], r, "right") - 1 clamped into [0, B), pos = r - cu[utt] clamped into
  [0, max_len): integers, exact.
* RoPE tables (`rope_ref`): ang = fl32(float(n) inv_freq[j]) — one IEEE multiplication (the kernel's __fmul_rn), reproduced exactly by
  torch's fp32 product — and cos / sin of THAT fp32 angle in fp64.  Bound: SINCOS_MULT times the measured floor (below), absolute.

What cannot be derived: the device's __expf inside silu_f and cosf / sinf at arguments of thousands of radians.  No constant is picked
for them.  `silu_floor` / `sincos_floor` measure, on the inputs of the case itself, the worst error of torch's CPU fp32 evaluation of
the same expression against fp64 (relative for silu, absolute for cos / sin, one scalar per case), and the kernel is allowed a fixed
multiple of it:
  SILU_MULT = 16.  silu_f(x) = x / (1 + __expf(-x)).  The CPU's expf is within 1 ulp and the floor (exponential, addition, division)
      comes to about 2 u.  The fast exponential is exp2(-x log2 e): rounding that product moves the argument by up to |x| log2(e) u,
      i.e. the exponential by the relative |x| log2(e) u — 6 u at |x| = 4 — on top of v_exp_f32's own ~1 ulp, the addition and the
      division (1 u each), in an association that differs from the CPU's.  About 10 u at the |x| <= 4 of the test data (the data
      keeps |pooled| and the time MLP's pre-activations there) against a floor of 2 u: 16 floors = 32 u covers it with a factor of
      three and leaves no room for a wrong term (a silu of the wrong element is off by O(1), 10^6 floors).
  SINCOS_MULT = 4.  A different but equally valid fp32 cosf / sinf (another argument reduction and polynomial, documented at <= 2 ulp
      against the CPU's < 1 ulp) errs by up to 2^-23 near |value| = 1, where the floor is about half an ulp, 2^-25 .. 2^-24.
Measured floors (CPU, this data): silu 1.374e-07 relative over the text modulation cases, 1.250e-07 over the time table cases; cos / sin
2.98e-08 (the format's own half ulp, N = 1), 3.557e-08 (N = 5), 3.581e-08 (N = 4099) absolute.
Measured on an MI355X (2026-10-19), the kernels' worst |kernel - reference| / bound over every case of test_gpu_rowwise.py (`pytest -s`
prints one ROW_RATIO line per case and output):
    AdaLN h                 0.657 dense, 0.661 packed   (the fp32 emulation: 0.661.  d = 64 rows: the statistics terms are small and
                                                         the final rounding, u |h| against half an ulp, is most of the bound)
    AdaLN u1, fp32 h        0.020 dense, 0.003 packed   (bitwise the LayerNorm launch as well)
    AdaLN u1, bf16 h        0.006 dense, 0.001 packed
    ditto_global_adaln h    0.021                       (t == NULL; the bound carries both modulation launches' bounds)
    finish out              bitwise the fp32 chain; the chain against fp64: 0.644
    finish u                0.001                       (bitwise the two-launch form as well)
    pooled                  0.507
    tmod                    0.014                       ((dt + 2) u |W| |s| dominates: correct sums err like sqrt(dt))
    time table              0.025
    RoPE cos / sin          0.476 / 0.468 over the table, 0.365 / 0.385 over the last 64 positions of N = 4099
u1, finish u, tmod and the time table sit at a few percent because their bounds are linear in the length of a sum whose order is not
promised; what keeps them sensitive is shown in test_rowwise_ref.py: every defect of its table leaves the bound on these very inputs.

The data (`adaln_case`, `finish_case`, `cond_case`, `time_case`): gpu_util.asym values; neighbouring rows' means and scales, and
neighbouring utterances' modulations and table rows, differ by decades (row_factors), so a row given its neighbour's utterance, table
row or statistics is wrong by orders of magnitude, not by rounding.
"""
import math

import numpy as np
import torch

import gemm_fp8_ref as F
import gemm_fr_ref as FR
from gemm_epi_ref import G, acc_bound, inv_freq                              # noqa: F401  (one copy of each)
from gemm_fp8_ref import LN_EPS, row_factors, worst_ratio                    # noqa: F401
from gpu_util import asym

SILU_MULT = 16
SINCOS_MULT = 4
SILU_SLOPE = 1.1          # max |silu'| = 1.0998
STEPS = 7

ADALN_D = [64, 772, 768, 1024, 1152, 2048]
DENSE_ROWS = [(1, 1), (3, 5), (2, 8)]
PACKED_LENS = [[1, 6, 3], [5, 5, 5]]
FINISH_SHAPES = [(1, 64), (5, 772), (7, 768), (9, 2048)]
FINISH_NSPLIT = [1, 2, 5]
COND_T = [1, 3, 4, 5, 9]
COND_DIMS = [(64, 64), (100, 65), (768, 768)]        # (dt, d): the three dt and the three d of the issue, paired
TIME_TD = [32, 300]
ROW_MAPS = {"one": [0, 9], "zero_len": [0, 3, 3, 7, 8, 20], "two_blocks": [0, 100, 256, 300]}
ROPE_N = [1, 5, 4099]


def bf16_bits(x):
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------ AdaLN ------------------------------------------------------------------
def adaln_case(utt, d, seed, steps=STEPS):
    """inputs of one AdaLN launch over len(utt) rows whose utterance indices are `utt` (dense: row // N): x with per-row mean and scale
    from row_factors, ttab [steps, 2d] and tmod [B, 2d] with per-row factors decades apart, t distinct per utterance with 0 and
    steps - 1 among them, g1 / be1 spread over three decades"""
    utt = torch.as_tensor(utt, dtype=torch.int64)
    M, B = utt.numel(), int(utt.max()) + 1
    sc, mu = row_factors(M, seed)[:, None], row_factors(M, seed + 1)[:, None]
    sign = torch.where(torch.arange(M)[:, None] % 2 == 0, 1.0, -1.0)
    x = (asym((M, d), seed) * sc + sign * mu).float()
    ttab = (asym((steps, 2 * d), seed + 2) * row_factors(steps, seed + 3)[:, None] * 0.3).float()
    tmod = (asym((B, 2 * d), seed + 4) * row_factors(B, seed + 5)[:, None] * 0.3).float()
    order = [0, steps - 1, 3, 5, 1, 2, 4]
    t = torch.tensor([order[b % len(order)] for b in range(B)], dtype=torch.int64)
    g1 = (1.0 + 0.5 * asym((d,), seed + 6)).float() * row_factors(d, seed + 7)
    be1 = (asym((d,), seed + 8) * row_factors(d, seed + 9)).float()
    return dict(x=x, ttab=ttab, tmod=tmod, t=t, utt=utt.to(torch.int32), g1=g1, be1=be1, steps=steps)


def dense_utt(B, N):
    return torch.arange(B * N) // N


def packed_utt(lens):
    return torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))


def adaln_ref(c, use_t=True, e_ttab=None, e_tmod=None):
    """(h64, bound) [M, d] of the module docstring; use_t False: the table row of utterance b is b (the t == NULL form).  e_ttab /
    e_tmod: bounds on tables the kernel read from another kernel's fp32 output (ditto_global_adaln), c["ttab"] / c["tmod"] then being
    their fp64 references: propagated as |t| (e_sc_t + e_sc_x) + e_sh_t + e_sh_x"""
    d = c["x"].shape[1]
    b = c["utt"].long()
    ts = c["t"][b] if use_t else b
    tt, tm = c["ttab"].double()[ts], c["tmod"].double()[b]
    t, rstd, em, er = F.layernorm_terms(c["x"])
    one_sc_t = 1.0 + tt[:, :d]
    scale, shift = one_sc_t + tm[:, :d], tt[:, d:] + tm[:, d:]
    h = t * scale + shift
    et = em * rstd + t.abs() * (er + 2 * G)
    es = G * (one_sc_t.abs() + scale.abs())
    e = scale.abs() * et + t.abs() * es + G * (t * scale).abs() + G * shift.abs() + G * h.abs() + 1e-30
    if e_ttab is not None:
        ett, etm = e_ttab[ts], e_tmod[b]
        e = e + (t.abs() + et) * (ett[:, :d] + etm[:, :d]) * (1 + 2 * G) + (ett[:, d:] + etm[:, d:]) * (1 + 2 * G)
    return h, e


def u1_ref(h_f32, g1, be1):
    """u1 of an fp32 h: the fp64 LayerNorm of the h the kernel stored, and the arithmetic bound before the bf16 grant"""
    return F.layernorm(h_f32, g1, be1)


def u1_ref_bf16_stream(h64, hb, g1, be1):
    """u1 of a bf16 h: LayerNorm64(h64) and the bound for a kernel that normalised an fp32 row within hb of h64"""
    return FR.layernorm_of_perturbed(h64, hb, g1, be1)


def adaln_emulate(c, use_t=True, h_bf16=False, mutate=None):
    """ln_kernel's AdaLN modes in torch fp32 (another association of the sums): dict(h, raw, u1).  mutate: a defect of the table in
    test_rowwise_ref.py"""
    x, d, M = c["x"], c["x"].shape[1], c["x"].shape[0]
    b = c["utt"].long()
    if mutate == "block_utt":
        b = b[torch.arange(M) // 4 * 4]
    ts = c["t"][b] if use_t and mutate != "t_is_b" else b.clamp_max(c["steps"] - 1)

    def stats(v, stats_of=None):
        s = v if stats_of is None else stats_of
        mean = s.mean(dim=1, keepdim=True)
        q = ((s - mean) ** 2).sum(dim=1, keepdim=True)
        var = q / (d - 1 if mutate == "unbiased" else d)
        return mean, torch.rsqrt(var + (0.0 if mutate == "no_eps" else 1e-5))

    mean, rstd = stats(x)
    tt, tm = c["ttab"][ts], c["tmod"][b]
    lo, hi = (slice(d, 2 * d), slice(0, d)) if mutate == "swap_halves" else (slice(0, d), slice(d, 2 * d))
    scale = (0.0 if mutate == "no_one" else 1.0) + tt[:, lo] + tm[:, lo]
    shift = tt[:, hi] + tm[:, hi]
    h = (x - mean) * rstd * scale + shift
    hn = h.to(torch.bfloat16).float() if mutate == "u1_from_bf16_h" else h
    mean1, rstd1 = stats(hn, x if mutate == "u1_stats_of_x" else None)
    u1 = ((hn - mean1) * rstd1 * c["g1"] + c["be1"]).to(torch.bfloat16)
    return dict(h=h.to(torch.bfloat16) if h_bf16 else h, raw=x.to(torch.bfloat16), u1=u1)


# --------------------------------------------------------------- split-K finish ---------------------------------------------------------------
def finish_case(M, N, nsplit, seed):
    """partials whose scales differ by decades between splits and rows, bias and residual, gamma / beta of the fused LayerNorm"""
    p = asym((nsplit, M, N), seed).float() * row_factors(nsplit, seed + 1)[:, None, None] * row_factors(M, seed + 2)[None, :, None]
    bias = (asym((N,), seed + 3) * row_factors(N, seed + 4)).float()
    res = (asym((M, N), seed + 5) * row_factors(M, seed + 6)[:, None]).float()
    gamma = (1.0 + 0.5 * asym((N,), seed + 7)).float() * row_factors(N, seed + 8)
    beta = (asym((N,), seed + 9) * row_factors(N, seed + 10)).float()
    return dict(p=p, bias=bias, res=res, gamma=gamma, beta=beta)


def finish_chain(p, bias=None, res=None, mutate=None):
    """the kernel's additions in torch fp32, in its order: bitwise its `out`"""
    n = p.shape[0] - (1 if mutate == "drop_last_split" else 0)
    acc = p[0].clone() if n > 0 else torch.zeros_like(p[0])
    for s in range(1, n):
        acc = acc + p[s]
    if bias is not None:
        if mutate == "bias_flat_index":       # bias4[i] with i the flat vector index: rows past the first read past the vector
            M, N = acc.shape
            far = torch.cat([bias, torch.full((M * N - N,), float("nan"))])
            acc = acc + far.reshape(M, N)
        else:
            acc = acc + bias
    if res is not None:
        acc = acc + res
    return acc


def finish_ref(p, bias=None, res=None):
    """(out64, bound): (nsplit + 2) u (sum |p_s| + |bias| + |residual|)"""
    out, S = p.double().sum(dim=0), p.double().abs().sum(dim=0)
    if bias is not None:
        out, S = out + bias.double(), S + bias.double().abs()
    if res is not None:
        out, S = out + res.double(), S + res.double().abs()
    return out, (p.shape[0] + 2) * G * S + 1e-30


def out2_image(out, ldo2, fill, mutate=None):
    """the [M, ldo2] bf16 buffer the kernel leaves: bf16(out) in the first N columns, `fill` elsewhere"""
    M, N = out.shape
    buf = torch.full((M * ldo2,), fill, dtype=torch.bfloat16)
    ld = N if mutate == "out2_stride_n" else ldo2
    idx = (torch.arange(M)[:, None] * ld + torch.arange(N)[None, :]).reshape(-1)
    buf[idx] = out.to(torch.bfloat16).reshape(-1)
    return buf.reshape(M, ldo2)


def layernorm_emulate(x, gamma, beta):
    """ln_kernel MODE 0 in torch fp32"""
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return ((x - mean) * torch.rsqrt(var + 1e-5) * gamma + beta).to(torch.bfloat16)


# ----------------------------------------------------------------- conditioning -----------------------------------------------------------------
def cond_lens(T):
    return [1, T, (T + 1) // 2]


def cond_case(T, dt, d, seed):
    """text [3, T, dt] with NaN in every padded row, lengths [1, T, (T + 1) // 2], the packed form of the same utterances, and the
    text_mlp weights; utterances' scales differ by decades (kept below |pooled| ~ 4: SILU_MULT's range)"""
    lens = cond_lens(T)
    B = len(lens)
    text = asym((B, T, dt), seed).float() * torch.tensor([0.05, 1.0, 0.3])[:, None, None] + torch.tensor([0.3, -0.5, 0.02])[:, None, None]
    for b, n in enumerate(lens):
        text[b, n:] = float("nan")
    packed = torch.cat([text[b, :n] for b, n in enumerate(lens)])
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    wx = (asym((2 * d, dt), seed + 1) / math.sqrt(dt)).float() * row_factors(2 * d, seed + 2)[:, None]
    bx = (asym((2 * d,), seed + 3) * row_factors(2 * d, seed + 4)).float()
    return dict(text=text, lens=torch.tensor(lens, dtype=torch.int32), packed=packed, cu=cu, wx=wx, bx=bx)


def pool_ref(rows):
    """(pooled64 [dt], bound) of the mean over rows [T_b, dt]"""
    r, n = rows.double(), rows.shape[0]
    return r.mean(dim=0), (n + 1) * G * r.abs().mean(dim=0) + 1e-30


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def silu32(x):
    return x / (1.0 + torch.exp(-x))


def silu_floor(z64):
    """the worst relative error of the CPU's fp32 silu against fp64 at the fp32 roundings of z64"""
    z = z64.float()
    want = silu64(z.double())
    return float(((silu32(z).double() - want).abs() / want.abs().clamp_min(1e-300)).max())


def silu_bound(z64, ez, floor):
    s = silu64(z64)
    return s, SILU_SLOPE * ez + SILU_MULT * floor * s.abs()


def linear_ref(W, v, ev, bias, K):
    """(W v + bias, bound): the propagated ev and K + 1 roundings (module docstring)"""
    W64, b64 = W.double(), bias.double()
    out = v @ W64.T + b64
    return out, ev @ W64.abs().T + acc_bound((v.abs() + ev) @ W64.abs().T + b64.abs(), K)


def text_mod_ref(c, floor=None):
    """(pooled64 [B, dt], pooled bound, tmod64 [B, 2d], tmod bound, floor): every utterance over its own rows"""
    pr = [pool_ref(c["text"][b, :int(n)]) for b, n in enumerate(c["lens"])]
    p, ep = torch.stack([a for a, _ in pr]), torch.stack([e for _, e in pr])
    floor = silu_floor(p) if floor is None else floor
    s, es = silu_bound(p, ep, floor)
    tmod, et = linear_ref(c["wx"], s, es, c["bx"], c["wx"].shape[1] + 1)
    return p, ep, tmod, et, floor


def pool_emulate(flat, starts, lens, T_div=None, mutate=None):
    """text_pool_kernel in torch fp32 over a flat [rows, dt] buffer: utterance b = rows [starts[b], starts[b] + lens[b])"""
    out = []
    for b, (s, n) in enumerate(zip(starts, lens)):
        s, n = int(s), int(n)
        if mutate == "packed_from_next_offset":
            s = s + n
        rows = flat[s:s + n + (1 if mutate == "one_row_past" else 0)]
        groups = [rows[g::4].sum(dim=0) if rows[g::4].numel() else torch.zeros(flat.shape[1]) for g in range(4)]
        div = T_div if mutate == "divide_by_T" else n
        out.append(((groups[0] + groups[1]) + (groups[2] + groups[3])) / float(div))
    return torch.stack(out)


def text_mod_emulate(pooled, wx, bx, mutate=None):
    s = pooled if mutate == "silu_missing" else silu32(pooled)
    return s @ wx.T + (bx.roll(-1) if mutate == "bias_of_next_row" else bx)


def time_case(td, d, seed, steps=3):
    emb = asym((steps, td), seed).float() * row_factors(steps, seed + 1)[:, None].clamp(0.05, 1.0)
    w = lambda n, k, s: (asym((n, k), s) / math.sqrt(k)).float()
    return dict(emb=emb, w0=w(td, td, seed + 2), b0=0.3 * asym((td,), seed + 3).float(), w2=w(td, td, seed + 4),
                b2=0.3 * asym((td,), seed + 5).float(), wt=w(2 * d, td, seed + 6) * row_factors(2 * d, seed + 7)[:, None],
                bt=(asym((2 * d,), seed + 8) * row_factors(2 * d, seed + 9)).float())


def time_table_ref(c):
    """(ttab64 [steps, 2d], bound, floor)"""
    td = c["emb"].shape[1]
    e = c["emb"].double()
    z1, ez1 = linear_ref(c["w0"], e, torch.zeros_like(e), c["b0"], td)
    z2_probe = silu64(z1) @ c["w2"].double().T + c["b2"].double()
    floor = max(silu_floor(z1), silu_floor(z2_probe))
    a, ea = silu_bound(z1, ez1, floor)
    z2, ez2 = linear_ref(c["w2"], a, ea, c["b2"], td)
    cc, ec = silu_bound(z2, ez2, floor)
    out, eo = linear_ref(c["wt"], cc, ec, c["bt"], td)
    return out, eo, floor


def time_table_emulate(c, mutate=None):
    emb = c["emb"].roll(-1, 0) if mutate == "embedding_of_next_step" else c["emb"]
    a = silu32(emb @ c["w0"].T + c["b0"])
    z2 = a @ c["w2"].T + c["b2"]
    cc = z2 if mutate == "second_silu_missing" else silu32(z2)
    return cc @ c["wt"].T + c["bt"]


# ------------------------------------------------------------------ row map ------------------------------------------------------------------
def row_map_ref(cu, max_len, mutate=None):
    """(utt, pos) int32 [S] for offsets cu [B + 1] (S = cu[-1])"""
    cu = np.asarray(cu, dtype=np.int64)
    B, S = len(cu) - 1, int(cu[-1])
    r = np.arange(S)
    side = "left" if mutate == "start_row_to_previous" else "right"
    utt = np.clip(np.searchsorted(cu[:B], r, side) - 1, 0, B - 1)
    if mutate == "zero_length_claims":      # the first of the utterances that start where the right one starts
        utt = np.searchsorted(cu[:B], cu[utt], "left")
    pos = np.clip(r - cu[utt], 0, max_len - 1)
    return torch.from_numpy(utt.astype(np.int32)), torch.from_numpy(pos.astype(np.int32))


# -------------------------------------------------------------------- RoPE --------------------------------------------------------------------
def rope_angles(N, invf, mutate=None):
    """fp32 [N, half]: fl32(float(n) * inv_freq[j]), torch's IEEE product"""
    half = invf.numel()
    n = torch.arange(N, dtype=torch.float32)[:, None]
    if mutate == "angle_from_flat_index":
        n = n * half + torch.arange(half, dtype=torch.float32)[None, :]
    return n * invf.float()[None, :]


def rope_ref(N, invf):
    """(cos64, sin64 [N, half], bound [N, half], floor): the bound is SINCOS_MULT floors, one scalar for the table"""
    ang = rope_angles(N, invf)
    a64 = ang.double()
    c, s = torch.cos(a64), torch.sin(a64)
    floor = float(torch.maximum((torch.cos(ang).double() - c).abs(), (torch.sin(ang).double() - s).abs()).max())
    floor = max(floor, 2.0 ** -25)           # N = 1: cos(0) = 1 and sin(0) = 0 are exact; half an ulp of 1 is the format's own floor
    return c, s, torch.full_like(c, SINCOS_MULT * floor), floor
