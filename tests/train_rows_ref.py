"""fp64 references, derived elementwise bounds, data and case tables for the backward pass's row kernels (csrc/train.hip,
csrc/train_packed.hip) behind the entries of include/ditto_train_rows.h, shared by test_train_rows_ref.py and test_train_rows_host.py
(no GPU) and test_gpu_train_rows.py.  In the manner of rowwise_ref.py and optim_ref.py: every function returns the expected value AND a
bound on |kernel - expected| computed from the inputs and the fp64 reference, never from the kernel's output.  u = 2^-24 (gemm_epi_ref.G).

* data (`scaled_rows`): asym times a per-row factor over 0.01 .. 30 in a shuffled order (gemm_fp8_ref.row_factors) plus a per-row mean of
  up to two of the row's scales: neighbouring rows' means and scales, and neighbouring utterances, differ by decades, so a row served
  with its neighbour's statistics, group or chunk is wrong by orders of magnitude (test_train_rows_ref.py's defect table).

* LayerNorm backward (`ln_bwd_ref`), all forms: g = dy gamma, dx = rstd (g - mean(g) - t mean(g t)), t = (x - mean) rstd.  The statistics'
  terms are gemm_fp8_ref.layernorm_terms' (em on the fp32 mean, er relative on the fp32 rstd): the kernel's xhat is within
      ext = em rstd + |t| (er + 2 u)
  of t.  m1 = mean(g): d additions and a division over g's own rounding: e1 = (d + 2) u mean|g|.  m2 = mean(g xhat):
  e2 = mean(|g| ext) + (d + 3) u mean(|g| (|t| + ext)).  The bracket g - m1 - xhat m2: ei = u |g| + e1 + ext |m2| + (|t| + ext) e2 + 3 u (|g| +
  |m1| + |t m2|).  dx32 = rstd32 * bracket: rstd ei + |dx| (er + u), and the addition into the accumulator one more rounding:
      e_dx = rstd ei + |dx| (er + u) + u |acc0 + dx|.
  dx_bf16 is not bounded: it is, bit for bit, the bf16 rounding of the dx_accum the kernel wrote.  dgamma = sum_r dy t, dbeta = sum_r dy:
  fp64 sums; rows addends in some fixed order: (rows + 1) u sum|.| (`colsum_ref`) plus, for dgamma, sum_r |dy| ext and the product's u.  The
  extra column sum is of the kernel's own dx_accum output (`colsum_ref` on it).  The per-utterance GlobalAdaLN reduction (`adaln_packed_ref`)
  is the same [dgamma | dbeta] over each utterance's own rows.

* gated-MLP derivative (`gated_ref`): da = dy sg (Phi(a) + a phi(a)), dg = dy a Phi(a) sg (1 - sg) with erf / exp exact in fp64.  The bound
  is half a bf16 ulp of the stored value (worst_ratio) plus an ABSOLUTE fp32 term, because 1 - sg cancels for large g and a phi + Phi cancels
  near a = -0.75 (a relative bound is wrong there):
      e_da = |dy sg| (|a| e_pdf + e_cdf) + |dy| |Phi + a phi| e_sg + 4 u |da|
      e_dg = |dy a| (e_cdf sg (1 - sg) + Phi e_sg + e_cdf e_sg + e_sg^2) + 5 u |dg|
  e_cdf = the rational form's error + the clamp's + its fp32 evaluation.  The first is computed HERE in fp64 from the kernel's coefficients
  (ERF_P, ERF_Q restate gated_bwd_elem) over z in [-4, 4] against math.erf (`erf_rational_error`), the second is erfc(4) / 2 (what is left
  of Phi beyond the clamp |z| = 4), the third CDF_ROUND u = 16 u: Horner steps of fmas on positive coefficients (relative 2 u per step over
  7 + 5 steps would be 24 u of Q; the quotient (Q + z P) / 2Q <= 1 divides by Q, and the measured fp32 emulation stays inside).
  e_pdf = GATED_MULT floors of phi, e_sg = GATED_MULT floors of sg, both ABSOLUTE (phi <= 0.4, sg <= 1).

* column sums (`colsum_ref`), the second stage alone, the fused bias sums of the gated kernel (fp64 sums of the bf16 dpre the kernel
  itself wrote — "what the wgrad GEMM will read"): (addends + 1) u sum|.|.

* transpose, pack_bf16_t, unpack_rows / vec, embedding scatter: exact (`transpose_ref`, `pack_map`, `scatter_ref`: the same fp32 additions
  in b order on the CPU, ids clamped into [0, V - 1]).

* dropout softmax rows (`softmax_rows_ref`): the mask is oracle.hash_dropout_mask's for (seed, layer, bh0 + row / rows_per_bh,
  row % rows_per_bh, j) and must agree exactly (zero against non-zero; the scores keep every probability above 1e-30).  With x = scale (S -
  max) the kernel's exponent argument (a subtraction, a product with the fp32 scale log2 e) is within 4 u |x| of x, the sum of Skv terms
  and the division add (Skv + 6) u:
      rel_j = 4 u (|x_j| + sum_k p_k |x_k|) + (Skv + 6) u + 2 EXP_MULT f_exp,      e_P = rel p keep / (1 - p_drop) + u |P|
  backward, g = dPd keep / (1 - p_drop), dsum = sum p g, dS = p (g - dsum) scale:
      e_dsum = sum_k (rel_k p_k |g_k|) + (Skv + 3) u sum_k p_k |g_k|
      e_dS = scale (rel p |g - dsum| + p (e_dsum + u (2 |g| + |dsum|))) + 3 u |dS|
  then half a bf16 ulp of the stored value.  Padding columns Skv .. ld - 1 are written as zero.

* small linear (`small_linear_ref`): as rowwise_ref.text_mod_ref: s = f(x) within SILU_MULT floors (relative; absolute for f'), a dot
  product of n products on a lane-strided loop: (ceil(n / 64) + 8) u sum|.| for the forward (64 lanes, 6 wave additions, the bias), (B + 1) u
  for the weight gradient's loop over b, (ceil(O / 4) + 4) u for the input gradient (four slices and their sum).

What cannot be derived: the device's v_exp_f32, v_rcp_f32 and rsqrtf inside gated_bwd_elem, the softmax rows and silu.  No constant is
picked for them.  As rowwise_ref.py does for silu, `floor32` measures on each case's own inputs the worst error of a torch-CPU fp32
evaluation of the same written expression against fp64, and the kernel is allowed a fixed multiple of it:
  GATED_MULT = EXP_MULT = 8.  v_exp_f32 and v_rcp_f32 are documented at 1 ulp each; sg = rcp(1 + exp2(g c)) adds the rounding of g c (the
      argument moves by u |g c|, sg by sg (1 - sg) ln 2 |g c| u <= 0.23 u), the addition and the reciprocal: about 3 u against a CPU floor of
      0.5 .. 1 u (floored at 2^-25, the format's own half ulp at 1), so 8 floors leave a factor of two to four and no room for a wrong term
      (every modelled defect is beyond 10^3 floors).  phi = c exp2(a^2 k): two roundings in the argument, |a^2 k| u ln 2 relative, 1 ulp of
      the exponential: the same reasoning on phi <= 0.4 (floor floored at 2^-27).  The softmax's exp2 likewise, relative.
  rowwise_ref.SILU_MULT = 16 for silu / silu' (its docstring).
rsqrtf is taken at gemm_fp8_ref.E_RSQRT_ULPS = 4 ulp inside layernorm_terms, as everywhere in the suite.

fp32 emulation of every kernel's written expression on every case of the tables (test_train_rows_ref.py, CPU), worst ratio per output:
LayerNorm dx_accum 0.883 (the accumulator's own rounding: half an ulp of a value just above 1 against u |acc|, which can reach 1 and no
more), dgamma 0.034, dbeta 0.432; adaln dmod 0.486; gated da 0.056, dg 0.123; softmax P 0.000 (inside half a bf16 ulp everywhere), dS
0.073; small linear 0.602; column sums 0.245.  Modelled defects, least ratio: the last ragged chunk dropped from the column sum of 9000
rows 9.1 (36 rows under a bound of 9001 u), mean(g) dropped 163, every other one above 500 (neighbour statistics 7e5, the gated bias sum
of unrounded values 1.1e3, gelu' without a phi 1.4e5, the mask of pair bh 1.6e5, mask not applied to dP 1.6e5).

Measured on an MI355X (2026-10-20), worst TROW_RATIO per output over all cases of test_gpu_train_rows.py:
  LayerNorm stream   dx_accum 0.883   dgamma 0.026   dbeta 0.399   colsum 0.398        (dx_bf16 bitwise)
  LayerNorm group    dx_accum 0.881   dgamma 0.025   dbeta 0.217
  adaln packed       dmod 0.400
  gated              da 0.055   dg 0.139   bias sums 0.271   rows 0-8 / 4088-4104 of (4104, 4096) 0.139
  column sums        0.234      second stage alone 0.332
  softmax rows       P 0.000    dS 0.073       (mask, padding columns exact)
  small linear       y 0.566    dW 0.602   dbias 0.328   dx 0.401
transpose, packers, unpackers and the scatter bit for bit; every pair of launches equal in bits; every guard pattern intact.  The
kernels sit where the CPU emulation does: no device instruction needed more than its floor's multiple.
"""
import math

import torch

import gemm_fp8_ref as F8
import rowwise_ref as RW
from gemm_epi_ref import G, worst_ratio  # noqa: F401
from gpu_util import asym

U = G
GATED_MULT = EXP_MULT = 8
CDF_ROUND = 16
BIG = 1 << 30     # "no blocks": the identity map of pack_bf16_t / unpack_*


def bf(x):
    """the bf16 rounding (nearest even) of fp32 / fp64 values, as bf16"""
    return x.float().to(torch.bfloat16)


def scaled_rows(rows, d, seed, mean=True):
    """fp32 [rows, d]: neighbouring rows' scales (and means) differ by decades"""
    s = F8.row_factors(rows, seed)[:, None]
    x = asym((rows, d), seed).float() * s
    if mean:
        x = x + s * (2.0 * asym((rows, 1), seed + 1).float().clamp(-1, 1))
    return x.contiguous()


def floor32(f32, f64, z, relative, least):
    """worst error of the CPU's fp32 evaluation f32(z) against f64(z) at the fp32 values z; relative or absolute; at least `least`"""
    z = z.float()
    want = f64(z.double())
    err = (f32(z).double() - want).abs()
    if relative:
        err = err / want.abs().clamp_min(1e-300)
    return max(float(err.max()), least)


def colsum_ref(x64, addends=None):
    """(sum over rows, bound): fp64 column sums of x64 [M, n] and (addends + 1) u sum|x|"""
    n = x64.shape[0] if addends is None else addends
    return x64.sum(0), (n + 1) * U * x64.abs().sum(0) + 1e-30


# ================================================================ LayerNorm backward ================================================================
LN_D = [64, 768, 772, 2048]
LN_ROWS = [1, 5, 37]
LN_STREAM_SHAPES = [(r, d) for d in LN_D for r in LN_ROWS] + [(1100, 64)]
LN_FORMS = [("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16")]          # (dy, x)
LN_GROUP_SHAPES = [(5, 3, 64), (33, 2, 772), (300, 70, 64)]             # (rows_per_group, groups, d)
ADALN_LENS = [[1, 6, 3], [5, 5, 5], [40, 1, 17]]
ADALN_D = [64, 772, 2048]


def ln_chunks(rows_per_group, groups):
    """restates ln_bwd_chunks (csrc/train.hip)"""
    return max(1, min((1024 + groups - 1) // groups, (rows_per_group + 15) // 16, 1024))


def ln_scratch_bytes(rows_per_group, groups, d):
    return groups * ln_chunks(rows_per_group, groups) * 3 * d * 4


def adaln_scratch_bytes(max_len, B, d):
    return B * max(1, min((1024 + B - 1) // B, (max_len + 15) // 16)) * 2 * d * 4


def ln_case(rows, d, seed, form=("f32", "f32")):
    """x, dy as the kernel gets them (fp32 or bf16), gamma, acc0 (the non-zero accumulator)"""
    x, dy = scaled_rows(rows, d, seed), scaled_rows(rows, d, seed + 3, mean=False)
    dy = bf(dy) if form[0] == "bf16" else dy
    x = bf(x) if form[1] == "bf16" else x
    return dict(x=x, dy=dy, gamma=(1 + 0.3 * asym((d,), seed + 5)).float().contiguous(), acc0=(0.5 * asym((rows, d), seed + 7)).float().contiguous())


def ln_bwd_ref(x, dy, gamma, acc0, segments=None):
    """x, dy [M, d] (any float dtype: the values the kernel read), gamma [d] or None, acc0 [M, d] or None (dx alone), segments: list of
    (lo, hi) row ranges of the [dgamma | dbeta] sums (default: all rows).  Returns dict(acc, e_acc [M, d]; dgamma, e_dgamma, dbeta, e_dbeta
    [len(segments), d])."""
    x, dy = x.double(), dy.double()
    M, d = x.shape
    t, rstd, em, er = F8.layernorm_terms(x)
    ext = em * rstd + t.abs() * (er + 2 * U)
    g = dy * (gamma.double() if gamma is not None else 1.0)
    mean = lambda v: v.mean(dim=1, keepdim=True)
    m1, m2 = mean(g), mean(g * t)
    dx = rstd * (g - m1 - t * m2)
    e1 = (d + 2) * U * mean(g.abs())
    e2 = mean(g.abs() * ext) + (d + 3) * U * mean(g.abs() * (t.abs() + ext))
    ei = U * g.abs() + e1 + ext * m2.abs() + (t.abs() + ext) * e2 + 3 * U * (g.abs() + m1.abs() + (t * m2).abs())
    a0 = acc0.double() if acc0 is not None else torch.zeros_like(dx)
    acc = a0 + dx
    out = dict(acc=acc, e_acc=rstd * ei + dx.abs() * (er + U) + U * acc.abs() + 1e-30)
    segments = segments or [(0, M)]
    dg, edg, db, edb = [], [], [], []
    for lo, hi in segments:
        n = hi - lo
        p = dy[lo:hi] * t[lo:hi]
        dg.append(p.sum(0))
        edg.append((dy[lo:hi].abs() * ext[lo:hi]).sum(0) + (n + 2) * U * (dy[lo:hi].abs() * (t[lo:hi].abs() + ext[lo:hi])).sum(0) + 1e-30)
        s, es = colsum_ref(dy[lo:hi])
        db.append(s)
        edb.append(es)
    out.update(dgamma=torch.stack(dg), e_dgamma=torch.stack(edg), dbeta=torch.stack(db), e_dbeta=torch.stack(edb))
    return out


def ln_bwd_emulate(x, dy, gamma, acc0, mutate=None):
    """the kernel's written expression in torch fp32 on the CPU (one rounding per operation, sums by torch): (acc, dgamma, dbeta [d]).
    mutate: 'neighbour_mean', 'neighbour_rstd' (row r served with row r + 1's statistic), 'no_mean_g' (mean(g) dropped)."""
    x, dy = x.float(), dy.float()
    d = x.shape[1]
    mean = x.sum(1, keepdim=True) / d
    dl = x - mean
    rstd = torch.rsqrt((dl * dl).sum(1, keepdim=True) / d + 1e-5)
    if mutate == "neighbour_mean":
        mean = mean.roll(-1, 0)
    if mutate == "neighbour_rstd":
        rstd = rstd.roll(-1, 0)
    xh = (x - mean) * rstd
    g = dy * gamma.float() if gamma is not None else dy
    m1 = g.sum(1, keepdim=True) / d
    m2 = (g * xh).sum(1, keepdim=True) / d
    if mutate == "no_mean_g":
        m1 = torch.zeros_like(m1)
    dx = rstd * (g - m1 - xh * m2)
    acc = acc0.float() + dx if acc0 is not None else dx
    return acc, (dy * xh).sum(0), dy.sum(0)


def adaln_case(lens, d, seed):
    """packed [S, d] rows: every utterance on its own scale (decades apart) on top of the rows' own"""
    S = sum(lens)
    f = F8.row_factors(len(lens), seed + 11)
    utt = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    x = scaled_rows(S, d, seed) * f[utt][:, None]
    dy = scaled_rows(S, d, seed + 3, mean=False) * f.flip(0)[utt][:, None]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return dict(x=x.contiguous(), dy=dy.contiguous(), cu=cu)


def adaln_packed_ref(c):
    """(dmod64 [B, 2d], bound)"""
    segs = list(zip(c["cu"][:-1], c["cu"][1:]))
    r = ln_bwd_ref(c["x"], c["dy"], None, None, segs)
    return torch.cat([r["dgamma"], r["dbeta"]], 1), torch.cat([r["e_dgamma"], r["e_dbeta"]], 1)


# ================================================================ gated-MLP derivative ================================================================
GATED_F = [16, 48, 512, 1024]
GATED_M = [1, 5, 33]
GATED_BIG = (4104, 4096)
GATED_A = [0.0, 0.75, 4 * math.sqrt(2.0), 8.0, 30.0]
GATED_G = [0.0, 20.0, 90.0]
ERF_P = [1.9217200275534196e-08, -1.990321152334218e-06, 0.00015553680714219809, 0.0042930529452860355, 0.05243346840143204,
         0.2139447033405304, 1.1283786296844482]                       # gated_bwd_elem's pn, highest power first
ERF_Q = [0.0010980380466207862, 0.01555109117180109, 0.12079962342977524, 0.5229312181472778, 1.0]


def _horner(c, u):
    r = torch.full_like(u, c[0])
    for k in c[1:]:
        r = r * u + k
    return r


def cdf_rational(a):
    """Phi(a) by the kernel's form in the dtype of `a`: z = clamp(a / sqrt 2, -4, 4), (Q + z P) / (2 Q)"""
    z = (a * 0.70710678118654752440).clamp(-4.0, 4.0)
    u = z * z
    p, q = _horner(ERF_P, u), _horner(ERF_Q, u)
    return (z * p + q) * (0.5 / q)


def erf_rational_error(extra_a=None):
    """max |rational Phi - Phi| in fp64 over z in [-4, 4] (65 537 points, and the case's own a), plus the clamp's erfc(4) / 2"""
    z = torch.linspace(-4.0, 4.0, 65537, dtype=torch.float64)
    a = z * math.sqrt(2.0)
    if extra_a is not None:
        a = torch.cat([a, extra_a.double().flatten().clamp(-4 * math.sqrt(2.0), 4 * math.sqrt(2.0))])
    want = 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0)))
    return float((cdf_rational(a) - want).abs().max()) + 0.5 * math.erfc(4.0)


def gated_case(M, F, seed):
    """a, g, dy as bf16 [M, F]: asym over a few units, the special points of the issue sprinkled over the first elements of each row, dy
    with per-row scales over decades"""
    a = 2.5 * asym((M, F), seed).float()
    g = 4.0 * asym((M, F), seed + 1).float()
    sa = torch.tensor([s * v for v in GATED_A for s in (1.0, -1.0)])
    sg = torch.tensor([s * v for v in GATED_G for s in (1.0, -1.0)])
    grid_a, grid_g = sa.repeat_interleave(len(sg)), sg.repeat(len(sa))          # every pair, 60 of them
    n = min(F, len(grid_a))
    for m in range(M):
        sh = (7 * m) % len(grid_a)
        a[m, :n], g[m, :n] = grid_a.roll(sh)[:n], grid_g.roll(sh)[:n]
    dy = scaled_rows(M, F, seed + 2, mean=False)
    return dict(a=bf(a), g=bf(g), dy=bf(dy))


def interleave(a, g):
    """[M, F] fc1 and gate values -> the packed [M, 2F] column order (blocks of 16)"""
    M, F = a.shape
    return torch.stack([a.view(M, F // 16, 16), g.view(M, F // 16, 16)], 2).reshape(M, 2 * F).contiguous()


phi64 = lambda a: torch.exp(-0.5 * a * a) * 0.39894228040143267794
sg64 = lambda g: 1.0 / (1.0 + torch.exp(-g))


def gated_ref(c):
    """(dpre64 [M, 2F] packed order, bound before the bf16 store, floors)"""
    a, g, dy = c["a"].double(), c["g"].double(), c["dy"].double()
    Phi, phi, sg = 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))), phi64(a), sg64(g)
    f_pdf = floor32(lambda z: torch.exp(-0.5 * z * z) * 0.39894228040143267794, phi64, c["a"], False, 2.0 ** -27)
    f_sg = floor32(lambda z: 1.0 / (1.0 + torch.exp(-z)), sg64, c["g"], False, 2.0 ** -25)
    e_pdf, e_sg = GATED_MULT * f_pdf, GATED_MULT * f_sg
    e_cdf = erf_rational_error(c["a"]) + CDF_ROUND * U
    gp = Phi + a * phi
    da = dy * sg * gp
    dg = dy * a * Phi * sg * (1.0 - sg)
    e_da = (dy * sg).abs() * (a.abs() * e_pdf + e_cdf) + dy.abs() * gp.abs() * e_sg + 4 * U * da.abs() + 1e-38
    e_dg = (dy * a).abs() * (e_cdf * sg * (1.0 - sg) + Phi * e_sg + e_cdf * e_sg + e_sg * e_sg) + 5 * U * dg.abs() + 1e-38
    return interleave(da, dg), interleave(e_da, e_dg), dict(pdf=f_pdf, sg=f_sg, cdf=e_cdf)


def gated_emulate(c, mutate=None):
    """gated_bwd_elem in torch fp32: (da, dg) [M, F] before the store.  mutate: 'no_a_pdf' (gelu' without a phi), 'sigmoid_sign'
    (1 + sg for 1 - sg)"""
    a, g, dy = c["a"].float(), c["g"].float(), c["dy"].float()
    cdf = cdf_rational(a)
    pdf = 0.39894228040143267794 * torch.exp2(a * a * -0.72134752044448170368)
    sg = 1.0 / (1.0 + torch.exp2(g * -1.4426950408889634))
    t = dy * sg
    da = t * (cdf if mutate == "no_a_pdf" else a * pdf + cdf)
    dg = t * (a * cdf) * ((1.0 + sg) if mutate == "sigmoid_sign" else (1.0 - sg))
    return da, dg


# ================================================================ column sums, transpose, maps ================================================================
COLSUM_CASES = [(1, 8, 8), (7, 260, 264), (33, 256, 768), (100, 264, 264), (9000, 16, 24)]        # (M, n, ld)
REDUCE_CASES = [(1, 5), (17, 33), (130, 40), (2, 65536), (32, 65540), (33, 65536), (2, 65538)]     # (chunks, n): the last two miss the 16-byte kernel's rule
TRANSPOSE_ROWS = [1, 63, 64, 65, 100]
TRANSPOSE_COLS = [8, 64, 72]
PACK_CASES = [(96, 40, 16, 2, 0), (96, 40, 16, 2, 16), (33, 35, BIG, 1, 0)]                       # (rows, cols, blk, mult, row_off)
UNPACK_CASES = [(96, 40, 16, 2, 0), (96, 40, 16, 2, 16), (33, 36, BIG, 1, 0)]                     # cols % 4 == 0: (33, 35, ..) is REFUSED


def colsum_chunks(M, n):
    """restates colsum_chunks (csrc/train.hip)"""
    return max(1, min(max(1, 1024 // ((n + 255) // 256)), 256, (M + 15) // 16))


def colsum_scratch_bytes(M, n):
    return colsum_chunks(M, n) * n * 4


def pack_map(rows, blk, mult, row_off=0, use_off=True):
    r = torch.arange(rows)
    return (r // blk) * (blk * mult) + r % blk + (row_off if use_off else 0)


def pack_ldT(rows, blk, mult, row_off):
    """the dst row length of a pack case: the map's range rounded up to 8"""
    return (int(pack_map(rows, blk, mult, row_off)[-1]) + 1 + 7) // 8 * 8


def transpose_ref(src, rows, cols, ldT):
    """src bf16 [rows, >= cols] -> [cols, ldT], zero padded"""
    out = torch.zeros(cols, ldT, dtype=src.dtype)
    out[:, :rows] = src[:rows, :cols].T
    return out


def scatter_case(V, d, seed):
    """B = 6: two duplicate pairs, one id below 0 and one above V - 1"""
    ids = torch.tensor([3, -3, 3, V + 2, 1, 1], dtype=torch.int64)
    return dict(ids=ids, drows=scaled_rows(6, d, seed, mean=False), table0=(0.25 * asym((V, d), seed + 1)).float().contiguous())


def scatter_ref(c, V, clamp=True, accumulate=True):
    """the same fp32 additions in b order"""
    t = c["table0"].clone()
    for b, i in enumerate(c["ids"].tolist()):
        i = min(max(i, 0), V - 1) if clamp else i % V
        t[i] = t[i] + c["drows"][b] if accumulate else c["drows"][b]
    return t


# ================================================================ dropout softmax rows ================================================================
SOFTMAX_SKV = [1, 63, 64, 65, 130]
SOFTMAX_RPB = [3, 5]
SOFTMAX_P = [0.0, 0.1]
SOFTMAX_PAIRS, SOFTMAX_BH0, SOFTMAX_SEED, SOFTMAX_LAYER, SOFTMAX_SCALE = 3, 2, 0x1234567887654321, 3, 0.125


def softmax_case(rpb, Skv, seed):
    nrows, ld = rpb * SOFTMAX_PAIRS, (Skv + 63) // 64 * 64
    f = F8.row_factors(nrows, seed)[:, None] * 4.0                              # scale (S - max) reaches -0.02 .. -60 per row
    S = torch.full((nrows, ld), float("nan"))
    S[:, :Skv] = asym((nrows, Skv), seed).float().clamp(-2, 2) * f + 3.0 * asym((nrows, 1), seed + 1).float()
    dP = torch.full((nrows, ld), float("nan"))
    dP[:, :Skv] = scaled_rows(nrows, Skv, seed + 2)
    return dict(S=S.contiguous(), dP=dP.contiguous(), nrows=nrows, ld=ld, Skv=Skv, rpb=rpb)


def softmax_mask(c, p, bh0=SOFTMAX_BH0):
    """keep mask fp64 [nrows, Skv] of the pairs bh0 .. from the oracle's streams"""
    from oracle.ditto_oracle import hash_dropout_mask
    if p == 0:
        return torch.ones(c["nrows"], c["Skv"], dtype=torch.float64)
    m = hash_dropout_mask(SOFTMAX_SEED, SOFTMAX_LAYER, 1, bh0 + SOFTMAX_PAIRS, c["rpb"], c["Skv"], p)
    return m[0, bh0:].reshape(c["nrows"], c["Skv"]).double()


def softmax_rows_ref(c, p, mask=None, mask_dp=None):
    """dict(P, e_P, dS, e_dS [nrows, ld] fp64, padding columns 0; keep [nrows, Skv]; floor).  mask / mask_dp override the masks of P and of
    dP (the defect table)."""
    Skv, sc = c["Skv"], SOFTMAX_SCALE
    keep = softmax_mask(c, p) if mask is None else mask
    keep_dp = keep if mask_dp is None else mask_dp
    ks = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32))) if p else 1.0
    S = c["S"][:, :Skv].double()
    x = (S - S.max(1, keepdim=True).values) * sc
    pr = torch.softmax(x, 1)
    assert float(pr.min()) > 1e-30
    f_exp = floor32(torch.exp, torch.exp, x, True, 2.0 ** -25)
    rel = 4 * U * (x.abs() + (pr * x.abs()).sum(1, keepdim=True)) + (Skv + 6) * U + 2 * EXP_MULT * f_exp
    P = pr * keep * ks
    e_P = rel * P + U * P + 1e-38
    g = c["dP"][:, :Skv].double() * keep_dp * ks
    dsum = (pr * g).sum(1, keepdim=True)
    dS = pr * (g - dsum) * sc
    e_dsum = (rel * pr * g.abs()).sum(1, keepdim=True) + (Skv + 3) * U * (pr * g.abs()).sum(1, keepdim=True)
    e_dS = sc * (rel * pr * (g - dsum).abs() + pr * (e_dsum + U * (2 * g.abs() + dsum.abs()))) + 3 * U * dS.abs() + 1e-38
    pad = lambda v, fill: torch.cat([v, torch.full((c["nrows"], c["ld"] - Skv), fill, dtype=torch.float64)], 1)
    return dict(P=pad(P, 0.0), e_P=pad(e_P, 1e-38), dS=pad(dS, 0.0), e_dS=pad(e_dS, 1e-38), keep=keep, floor=f_exp)


def softmax_emulate(c, p, keep, keep_dp=None):
    """both kernels' written expressions in torch fp32: (P, dS) [nrows, Skv] before the store"""
    Skv = c["Skv"]
    keep_dp = keep if keep_dp is None else keep_dp
    sl2 = torch.tensor(SOFTMAX_SCALE, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    ks = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)) if p else torch.tensor(1.0)
    S = c["S"][:, :Skv]
    e = torch.exp2((S - S.max(1, keepdim=True).values) * sl2)
    pr = e * (1.0 / e.sum(1, keepdim=True))
    g = c["dP"][:, :Skv] * keep_dp.float() * ks
    dsum = (pr * g).sum(1, keepdim=True)
    return pr * keep.float() * ks, pr * (g - dsum) * SOFTMAX_SCALE


# ================================================================ small linear ================================================================
SMALL_LINEAR_CASES = [(1, 1, 1), (3, 65, 5), (2, 300, 7), (5, 64, 130)]          # (B, I, O)

silu_grad64 = lambda x: torch.sigmoid(x) * (1.0 + x * (1.0 - torch.sigmoid(x)))


def small_linear_case(B, I, O, seed):
    return dict(x=(2.0 * scaled_rows(B, I, seed, mean=False).clamp(-20, 20)).contiguous(), W=(scaled_rows(O, I, seed + 1, mean=False) / math.sqrt(I)).contiguous(),
                bias=(0.1 * asym((O,), seed + 2)).float().contiguous(), dy=scaled_rows(B, O, seed + 3, mean=False))


def small_linear_ref(c, mode, silu, bias=True):
    """mode 0: (y, e_y); 1: (dW, e_dW, dbias, e_dbias); 2: (dx, e_dx)"""
    x, W, dy = c["x"].double(), c["W"].double(), c["dy"].double()
    B, I = x.shape
    O = W.shape[0]
    if silu:
        s = RW.silu64(x)
        es = RW.SILU_MULT * RW.silu_floor(x) * s.abs()
    else:
        s, es = x, torch.zeros_like(x)
    if mode == 0:
        y = s @ W.T + (c["bias"].double() if bias else 0.0)
        return y, ((I + 63) // 64 + 8) * U * (s.abs() @ W.abs().T) + es @ W.abs().T + U * y.abs() + 1e-30
    if mode == 1:
        dW = dy.T @ s
        db, edb = colsum_ref(dy)
        return dW, (B + 1) * U * (dy.abs().T @ s.abs()) + dy.abs().T @ es + 1e-30, db, edb
    acc = dy @ W
    e_acc = ((O + 3) // 4 + 4) * U * (dy.abs() @ W.abs())
    if not silu:
        return acc, e_acc + 1e-30
    fp = silu_grad64(x)
    sig32 = lambda z: torch.sigmoid(z) * (1.0 + z * (1.0 - torch.sigmoid(z)))
    fg = floor32(sig32, silu_grad64, x, False, 2.0 ** -25)
    dx = fp * acc
    return dx, fp.abs() * e_acc + RW.SILU_MULT * fg * acc.abs() + U * dx.abs() + 1e-30


def small_linear_emulate(c, mode, silu, bias=True):
    x, W, dy = c["x"], c["W"], c["dy"]
    s = RW.silu32(x) if silu else x
    if mode == 0:
        return s @ W.T + (c["bias"] if bias else 0.0)
    if mode == 1:
        return dy.T @ s, dy.sum(0)
    acc = dy @ W
    return acc * (torch.sigmoid(x) * (1.0 + x * (1.0 - torch.sigmoid(x)))) if silu else acc


# ================================================================ one valid argument set per entry ================================================================
class Buf:
    """a device buffer of an argument set: `nbytes` exactly what the entry needs, `align` the alignment it demands; materialised as a
    fake address (test_train_rows_host.py: refused calls only) or a real allocation (test_gpu_train_rows.py: the valid call)"""

    def __init__(self, nbytes, align, optional=False):
        self.nbytes, self.align, self.optional = int(nbytes), align, optional


def host_arg_sets():
    """label -> (entry, arguments by the header's names with a Buf for every pointer (its `<name>_bytes` follows from it), [(overrides,
    expected status)]: each shape / argument rule of the entry broken alone).  The shapes are cases of the tables above."""
    SH, AR = 2, 1                                                           # hip.ERR_SHAPE, hip.ERR_ARG
    sets = {}
    rows, d = 37, 772
    n = rows * d
    sets["ln_stream"] = ("ditto_bwd_ln_stream", dict(
        dy=Buf(n * 2, 8), dy_bf16=1, x=Buf(n * 2, 8), x_bf16=1, gamma=Buf(d * 4, 16, True), dx_accum=Buf(n * 4, 16), dx_bf16=Buf(n * 2, 8),
        dgamma=Buf(d * 4, 4, True), dbeta=Buf(d * 4, 4, True), colsum=Buf(d * 4, 4, True), scratch=Buf(ln_scratch_bytes(rows, 1, d), 16),
        rows=rows, d=d, stream=None),
        [(dict(d=770), SH), (dict(d=2052), SH), (dict(d=0), SH), (dict(rows=0), SH), (dict(dy_bf16=0), SH), (dict(x_bf16=2), SH)])
    lens, d = ADALN_LENS[2], 64
    S, B = sum(lens), len(lens)
    sets["adaln_packed"] = ("ditto_bwd_adaln_packed", dict(
        dy=Buf(S * d * 4, 16), x=Buf(S * d * 4, 16), cu=Buf((B + 1) * 4, 4), dmod=Buf(B * 2 * d * 4, 4),
        scratch=Buf(adaln_scratch_bytes(max(lens), B, d), 16), B=B, S=S, max_len=max(lens), d=d, stream=None),
        [(dict(B=0), SH), (dict(B=65536), SH), (dict(max_len=S + 1), SH), (dict(max_len=0), SH), (dict(d=66), SH), (dict(S=0), SH)])
    M, F = 33, 512
    sets["gated"] = ("ditto_bwd_gated", dict(
        dact=Buf(M * F * 2, 16), pre=Buf(M * F * 4, 16), dpre=Buf(M * F * 4, 16), colsum=Buf(2 * F * 4, 4, True),
        scratch=Buf(256 * 2 * F * 4, 16, True), M=M, F=F, stream=None),
        [(dict(F=24), SH), (dict(F=0), SH), (dict(M=0), SH), (dict(colsum=None), AR), (dict(scratch=None), AR)])
    M, n, ld = COLSUM_CASES[1]
    sets["colsum"] = ("ditto_bwd_colsum", dict(
        x=Buf(((M - 1) * ld + n) * 2, 8), x_bf16=1, out=Buf(n * 4, 4), scratch=Buf(colsum_scratch_bytes(M, n), 16), M=M, n=n, ld=ld, stream=None),
        [(dict(n=262), SH), (dict(ld=262), SH), (dict(ld=256), SH), (dict(M=0), SH), (dict(n=0), SH), (dict(x_bf16=2), SH)])
    chunks, n = REDUCE_CASES[1]
    sets["reduce_partials"] = ("ditto_bwd_reduce_partials", dict(
        partial=Buf(chunks * n * 4, 16), out=Buf(n * 4, 16), chunks=chunks, n=n, stream=None), [(dict(chunks=0), SH), (dict(n=0), SH)])
    rows, cols, nzo, nzi, ldT = 65, 72, 2, 3, 128
    ld, s_o, d_z = nzi * cols, rows * nzi * cols, cols * ldT
    sets["transpose"] = ("ditto_bwd_transpose_bf16", dict(
        src=Buf(((nzo - 1) * s_o + (nzi - 1) * cols + (rows - 1) * ld + cols) * 2, 16), dst=Buf(nzo * nzi * d_z * 2, 16), rows=rows, cols=cols,
        ld=ld, ldT=ldT, nz_o=nzo, nz_i=nzi, s_o=s_o, s_i=cols, d_z=d_z, stream=None),
        [(dict(cols=76), SH), (dict(cols=0), SH), (dict(ld=220), SH), (dict(ld=64), SH), (dict(ldT=96), SH), (dict(ldT=64), SH), (dict(rows=0), SH),
         (dict(nz_o=0), SH), (dict(nz_i=0), SH), (dict(nz_o=65535), SH), (dict(s_o=s_o + 4), SH), (dict(s_i=cols + 4), SH), (dict(d_z=d_z + 4), SH),
         (dict(d_z=d_z - 8), SH)])
    rpb, Skv = 5, 65
    nrows, ld = rpb * SOFTMAX_PAIRS, 128
    soft = dict(nrows=nrows, rows_per_bh=rpb, Skv=Skv, ld=ld, scale=SOFTMAX_SCALE, seed=SOFTMAX_SEED, layer=SOFTMAX_LAYER, bh0=SOFTMAX_BH0,
                p_drop=0.1, stream=None)
    soft_bad = [(dict(Skv=129), SH), (dict(Skv=0), SH), (dict(rows_per_bh=0), SH), (dict(nrows=0), SH), (dict(bh0=-1), SH), (dict(layer=-1), SH),
                (dict(p_drop=1.0), SH), (dict(p_drop=-0.1), SH), (dict(scale=math.inf), SH)]
    fin = ((nrows - 1) * ld + Skv) * 4
    sets["softmax_drop_rows"] = ("ditto_bwd_softmax_drop_rows", dict(S=Buf(fin, 4), P=Buf(nrows * ld * 2, 2), **soft), soft_bad)
    sets["softmax_rows"] = ("ditto_bwd_softmax_rows", dict(S=Buf(fin, 4), dPd=Buf(fin, 4), dS=Buf(nrows * ld * 2, 2), **soft), soft_bad)
    B, I, O = SMALL_LINEAR_CASES[1]
    xb, wb, yb, ob = Buf(B * I * 4, 4), Buf(O * I * 4, 4), Buf(B * O * 4, 4), Buf(O * 4, 4, True)
    lin_bad = [(dict(mode=3), SH), (dict(mode=-1), SH), (dict(B=0), SH), (dict(I=0), SH), (dict(O=65536), SH), (dict(silu_in=2), SH)]
    lin = dict(B=B, I=I, O=O, silu_in=1, stream=None)
    sets["small_linear_fwd"] = ("ditto_bwd_small_linear", dict(mode=0, x=xb, W=wb, dy=None, out=yb, bias=ob, **lin), lin_bad + [(dict(dy=yb), AR)])
    sets["small_linear_bwd_w"] = ("ditto_bwd_small_linear", dict(mode=1, x=xb, W=None, dy=yb, out=wb, bias=ob, **lin), lin_bad + [(dict(W=wb), AR)])
    sets["small_linear_bwd_x"] = ("ditto_bwd_small_linear", dict(mode=2, x=xb, W=wb, dy=yb, out=xb, bias=None, **lin), lin_bad + [(dict(bias=ob), AR)])
    B, V, d = 6, 5, 300
    sets["scatter"] = ("ditto_bwd_embedding_scatter_add", dict(
        drows=Buf(B * d * 4, 4), ids=Buf(B * 8, 8), dtable=Buf(V * d * 4, 4), B=B, V=V, d=d, stream=None), [(dict(V=0), SH), (dict(B=0), SH), (dict(d=0), SH)])
    rows, cols, blk, mult, off = PACK_CASES[1]
    last, ldT = int(pack_map(rows, blk, mult, off)[-1]), pack_ldT(rows, blk, mult, off)
    map_bad = [(dict(blk=0), SH), (dict(mult=0), SH), (dict(row_off=-1), SH), (dict(rows=0), SH)]
    sets["pack_bf16_t"] = ("ditto_bwd_pack_bf16_t", dict(
        src=Buf(rows * cols * 4, 4), dst=Buf(((cols - 1) * ldT + last + 1) * 2, 2), rows=rows, cols=cols, ldT=ldT, blk=blk, mult=mult, row_off=off,
        stream=None), map_bad + [(dict(ldT=last), SH), (dict(cols=0), SH)])
    sets["unpack_rows"] = ("ditto_bwd_unpack_rows", dict(
        src=Buf((last + 1) * cols * 4, 16), dst=Buf(rows * cols * 4, 16), rows=rows, cols=cols, blk=blk, mult=mult, row_off=off, stream=None),
        map_bad + [(dict(cols=42), SH), (dict(cols=0), SH)])
    sets["unpack_vec"] = ("ditto_bwd_unpack_vec", dict(
        src=Buf((last + 1) * 4, 4), dst=Buf(rows * 4, 4), rows=rows, blk=blk, mult=mult, row_off=off, stream=None), map_bad)
    return sets


def materialise(args, address):
    """keyword arguments of hip.call from an argument set; address(Buf) -> int"""
    kw = {}
    for k, v in args.items():
        if isinstance(v, Buf):
            kw[k], kw[k + "_bytes"] = address(v), v.nbytes
        elif v is None and k != "stream":
            kw[k], kw[k + "_bytes"] = None, 0
        else:
            kw[k] = v
    return kw
