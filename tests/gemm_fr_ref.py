"""fp64 references and elementwise error bounds for the full-row GEMM family (csrc/gemm_frd.hip, csrc/gemm_fr64.hip, csrc/gemm_lnq.hip
and their shared csrc/fr_common.h) and the stand-alone LayerNorm launches they claim to match, shared by test_gemm_fr_ref.py (no GPU)
and test_gpu_gemm_fr.py.  Plain torch on the operands the kernel saw; every function returns the expected value AND a bound on
|kernel - expected| derived from the kernel's arithmetic, never a fitted constant.  linear / acc_bound / ulp32 / G are gemm_epi_ref's,
layernorm_terms / layernorm / row_factors / worst_ratio gemm_fp8_ref's; the project's own LayerNorm kernel appears in no reference.
u = 2^-24 below; K is the contraction length, d the row width.

* h (`h_ref`): h64 = residual + A W^T + bias.  The accumulators start from fl32(residual + bias) (fr_acc_init: one rounding of a
  value <= |residual| + |bias|), then the MFMAs add K products of bf16 values (exact in fp32) in fp32 in some order: K additions,
  each rounding a partial sum <= |residual| + |bias| + |A| |W|^T.  With the epilogue reading the accumulators as they are:
      |h32 - h64| <= (K + 2) u (|A| |W|^T + |bias| + |residual|)                                            (acc_bound at K + 1).
  bf16 stream (fr_hb): the stored h is the bf16 rounding of that h32: half a bf16 ulp of the stored value on top
  (worst_ratio(stored="bf16")).
* u, fp32 stream (`layernorm`): the kernel normalises the accumulators, whose values ARE the fp32 h it stores, so the reference is
  the fp64 LayerNorm of the kernel's own h output (which the h assertion of the same case pins elementwise).  The bound is
  gemm_fp8_ref.layernorm's (mean em, variance ev, rstd er, the subtraction, the multiplication, the fma: derived there; the order of
  the row sums does not enter it: per half row and lane in gemm_fr64, per quarter row in gemm_frd, per wave in the row kernels)
  plus ONE more rounding u |gamma t| for the forms that are written (v - mean) * rstd * g + b and may not be contracted into an fma
  (gemm_frd / gemm_fr64 epilogue, ln_dual_kernel).  gemm_fr64 / gemm_frd take the deviations of the variance pass as
  fma(sum, -1 / d, v): one rounding instead of two, inside the same term.  Then the bf16 or e4m3 store grant.
* u, bf16 stream (`layernorm_of_perturbed`): the kernel normalises the UNROUNDED fp32 row x32 = h64 + dx, |dx| <= hb (the h bound),
  but stores only bf16(x32), so the reference is LayerNorm64(h64) and dx is propagated.  With m, v the row's mean and biased variance,
  s = v + eps, r = s^-1/2, t_i = (x_i - m) r:   dm = mean(dx);   dv = 2 mean((x - m) dx) + mean((dx - dm)^2) exactly (the
  deviations sum to 0);   delta = dv / s;   r' = r (1 + delta)^-1/2.   2 mean((x - m) dx) / s = 2 r mean(t dx), so
      t'_i - t_i = t_i ((1 + delta)^-1/2 - 1) + (dx_i - dm) r (1 + delta)^-1/2
                 = [ r (dx_i - dm) - t_i r mean(t dx) ]  +  R_i,
      first order:   |.| <= r (|dx_i| + mean|dx| + |t_i| mean(|t| |dx|)),
      remainder:     R_i = t_i ((1 + delta)^-1/2 - 1 + delta / 2 - delta2 / 2) + (dx_i - dm) r ((1 + delta)^-1/2 - 1),
                     delta2 = mean((dx - dm)^2) / s <= r^2 mean(dx^2),   |delta| <= db = 2 r mean(|t| |dx|) + r^2 mean(dx^2).
  For |delta| <= 1/2 Taylor's remainder gives |(1 + delta)^-1/2 - 1 + delta / 2| <= (3 / 8) (1/2)^-5/2 delta^2 < 2.2 delta^2 and
  |(1 + delta)^-1/2 - 1| <= |delta| (0.414 at delta = -1/2), so
      |R_i| <= |t_i| (2.2 db^2 + r^2 mean(dx^2) / 2) + r (|dx_i| + mean|dx|) db            (db > 1/2: no bound, ratio inf).
  |u - u64| <= |gamma| |dt| + the arithmetic bound above.  That bound is evaluated at h64 while the kernel ran on x32: its mean term
  grows by at most (d + 1) u mean|dx| r, its |t| by |dt|, and its terms in 1 / (v + eps) and r by at most 1 / (1 - db) <= 1 + 2 db.
* lnq (`lnq_ref`): y64 = LayerNorm64(h) gamma + beta on the rows the kernel read (fp32, or the bf16 values).  The kernel's y32 is
  within e_ln (the arithmetic bound; its LayerNorm is ln_kernel's statement for statement, fma form) and is rounded to bf16 in the
  LDS: half a bf16 ulp <= 2^-8 |y32| (equality just above a power of two), so every A element of the product is within
      e_k = e_ln_k + 2^-8 (|y_k| + e_ln_k).
  out64 = y64 W^T + bias;  the MFMAs add K products in fp32 and the epilogue adds the fp32 bias:
      |out32 - out64| <= e |W|^T + (K + 1) u ((|y| + e) |W|^T + |bias|),          then the bf16 store grant.
  With W = identity the fp32 sum has ONE non-zero term and a zero bias changes nothing: out IS bf16(y32), one rounding, and is
  checked against y64 within e_ln alone plus the store grant (`layernorm`), where a second rounding would show.
* exact integers (`exact_operands`): A in [-3, 3], W in [-2, 2], bias multiples of 2^-4 in [-4, 4], residual integers in [-8, 8]:
  every partial sum is a multiple of 2^-4 below 6 K + 12 < 2^20: exact in fp32 in any order, so h32 == h64 bit for bit, and
  bf16(h64) in the bf16 stream.  u is left to the bound there: rstd = (v + 1e-5)^-1/2 is a power of two for no representable row
  (1e-5 is not a dyadic number), so no row makes u == bf16(t) an exact statement.

The data (`case`): A from asym, W scaled 1 / sqrt(K); bias, gamma, beta spread over three decades in a shuffled order (row_factors),
so a vector read from the wrong 256-column piece or the wrong wave's columns is wrong by decades; the residual a hash of (row,
column) (`hashed_residual`, fp32 or bf16-exact); and the LAST FOUR rows of every case are the special rows of `special_rows` (their A
rows are zero and their residual is the row minus the bias, so h is that row up to one rounding).
"""
import math

import torch

import gemm_fp8_ref as F
from gemm_epi_ref import G, linear, acc_bound, ulp32                                           # noqa: F401  (one copy of each)
from gemm_fp8_ref import E_RSQRT_ULPS, LN_EPS, row_factors, worst_ratio, e4m3_edges, deq       # noqa: F401

N_SPECIAL = 4


# ------------------------------------------------------------------ data ------------------------------------------------------------------
def pack_w(W):
    """nn.Linear image [N, K] -> the stage-major image the full-row kernels stream: Wp[K / 16][N][16]"""
    N, K = W.shape
    return W.view(N, K // 16, 16).permute(1, 0, 2).contiguous()


def hashed_residual(M, N, bf16_exact=True):
    """fp32 [M, N] from a hash of the element's (row, column): sign, one of seven binades in [2^-5, 4) and seven mantissa bits
    (bf16_exact: every value exact in bf16) or all 23 (the fp32 stream)"""
    r = torch.arange(M, dtype=torch.int64).view(M, 1)
    c = torch.arange(N, dtype=torch.int64).view(1, N)
    k = (r * N + c) * 2654435761 % (1 << 32)
    k = (k ^ (k >> 15)) * 2246822519 % (1 << 32)
    k = k ^ (k >> 13)
    bits = (((k & 1) << 15) | ((127 - 5 + (k >> 8) % 7) << 7) | ((k >> 1) & 127)) << 16
    if not bf16_exact:
        bits = bits | ((k >> 16) & 0xFFFF)
    return bits.to(torch.int32).view(torch.float32).contiguous()


def special_rows(N, seed):
    """fp32 [4, N]: a constant row (variance 0: u == beta within the bound); |x - mean| ~ 1e-3 (variance ~ 1e-6: eps = 1e-5 dominates);
    mean 300 with spread 1; columns below and from N / 2 on with means -2 and +3 (a half-row or quarter-row statistic shows)"""
    from gpu_util import asym
    a = asym((3, N), seed).float()
    rows = torch.empty(N_SPECIAL, N)
    rows[0] = 1.75
    rows[1] = 0.5 + 1e-3 * a[0]
    rows[2] = 300.0 + a[1]
    rows[3] = a[2] + torch.where(torch.arange(N) < N // 2, -2.0, 3.0)
    return rows


def affine(N, seed, gscale=1.0):
    """(bias, gamma, beta) fp32 [N], each times its own shuffled three decades"""
    from gpu_util import asym
    bias = 0.1 * asym((N,), seed + 2) * row_factors(N, seed + 7)
    gamma = gscale * (1 + 0.5 * asym((N,), seed + 3)) * row_factors(N, seed + 8)
    beta = 0.1 * asym((N,), seed + 4) * row_factors(N, seed + 9)
    return bias.float().contiguous(), gamma.float().contiguous(), beta.float().contiguous()


def case(M, N, K, seed, stream="f32", gscale=1.0):
    """dict A bf16 [M, K], W bf16 [N, K], bias / gamma / beta fp32 [N], res fp32 [M, N] (stream "bf16": bf16-exact values); the last
    four rows are the special rows"""
    from gpu_util import asym
    assert M > N_SPECIAL
    A = asym((M, K), seed).to(torch.bfloat16)
    A[M - N_SPECIAL:] = 0
    W = (asym((N, K), seed + 1) / math.sqrt(K)).to(torch.bfloat16)
    bias, gamma, beta = affine(N, seed, gscale)
    res = hashed_residual(M, N, bf16_exact=stream == "bf16")
    res[M - N_SPECIAL:] = special_rows(N, seed + 5) - bias
    if stream == "bf16":
        res = res.to(torch.bfloat16).float()
    return dict(A=A.contiguous(), W=W.contiguous(), bias=bias, gamma=gamma, beta=beta, res=res.contiguous())


def exact_operands(M, N, K, seed):
    """the exact-integer family of the module docstring, same keys as `case` (no gamma / beta: `affine` serves)"""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    W = torch.randint(-2, 3, (N, K), generator=g).to(torch.bfloat16)
    bias = torch.randint(-64, 65, (N,), generator=g).float() / 16
    res = torch.randint(-8, 9, (M, N), generator=g).float()
    return dict(A=A, W=W, bias=bias, res=res)


def lnq_rows(M, d, seed, bf16_rows=False):
    """rows for the LayerNorm in front of a product, fp32 [M, d] (bf16_rows: bf16-exact values): asym * 1.7 + 0.4 with per-row scales
    over three decades, and from M = 5 on the special rows last"""
    from gpu_util import asym
    x = ((asym((M, d), seed) * 1.7 + 0.4) * row_factors(M, seed + 1)[:, None]).float()
    if M > N_SPECIAL:
        x[M - N_SPECIAL:] = special_rows(d, seed + 5)
    if bf16_rows:
        x = x.to(torch.bfloat16).float()
    return x.contiguous()


# --------------------------------------------------------------- references ---------------------------------------------------------------
def h_ref(A, W, bias=None, res=None):
    """(h64, bound) [M, N]: residual + A W^T + bias and (K + 2) u (|A| |W|^T + |bias| + |residual|)"""
    acc, absacc = linear(A, W, bias)
    if res is not None:
        acc, absacc = acc + res.double(), absacc + res.double().abs()
    return acc, acc_bound(absacc, A.shape[1] + 1)


def layernorm(x, gamma=None, beta=None):
    """fp64 LayerNorm of the rows x (the values the kernel normalised) and the arithmetic bound of the module docstring, before the
    store grant"""
    y, e = F.layernorm(x, gamma, beta)
    gt = y - beta.double() if beta is not None else y
    return y, e + G * gt.abs()


def layernorm_of_perturbed(h64, hb, gamma, beta):
    """the bf16 stream's u: LayerNorm64(h64) and the bound for a kernel that normalised h64 + dx, |dx| <= hb, in fp32"""
    d = h64.shape[1]
    y, e = layernorm(h64, gamma, beta)
    t, r, _, er = F.layernorm_terms(h64)
    ta, g = t.abs(), gamma.double().abs()
    mdx = hb.mean(dim=1, keepdim=True)
    mtdx = (ta * hb).mean(dim=1, keepdim=True)
    mdx2 = (hb * hb).mean(dim=1, keepdim=True)
    db = 2 * r * mtdx + r * r * mdx2
    first = r * (hb + mdx + ta * mtdx)
    rem = ta * (2.2 * db * db + r * r * mdx2 / 2) + r * (hb + mdx) * db
    dt = first + torch.where(db <= 0.5, rem, torch.full_like(rem, math.inf))
    moved = e * (1 + 2 * db) + g * (dt * (er + 3 * G) + (d + 1) * G * mdx * r)
    return y, g * dt + moved


def lnq_ref(h, gamma, beta, W, bias=None):
    """(out64, bound) [M, d] of (LayerNorm(h) gamma + beta) W^T + bias with the normalised rows rounded to bf16 on the way"""
    y, e_ln = layernorm(h, gamma, beta)
    e = e_ln + 2.0 ** -8 * (y.abs() + e_ln)
    W64 = W.double()
    out, absacc = y @ W64.T, (y.abs() + e) @ W64.abs().T
    if bias is not None:
        out, absacc = out + bias.double(), absacc + bias.double().abs()
    return out, e @ W64.abs().T + acc_bound(absacc, W.shape[1])
