"""fp64 references and elementwise error bounds for the fp8 (OCP e4m3) GEMM family and its two row kernels (csrc/gemm256.hip
gemm256_kernel<EPI, true, true, FLAT>, csrc/rowwise.hip ln_kernel<CH, 2> and pack_fp8_kernel), shared by test_gemm_fp8_ref.py (no
GPU) and test_gpu_gemm_fp8.py.  Plain torch on the DEQUANTISED bytes the kernel saw (torch.float8_e4m3fn is the same format); every
function returns the expected value AND a bound on |kernel - expected| derived from the kernel's arithmetic, never a fitted
constant.  rope / rope_bound, gated / gated_bound, ulp32 and dtheta_table_free are gemm_epi_ref's.  The terms:

* accumulation (`linear`): acc64 = (A Wq^T) wscale[n] + bias.  A product of two e4m3 values has 8 significant bits: exact in fp32.
  Were the MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, both scales 1) to add the K products in fp32 in some order, the term would be
      (K + 2) 2^-24 (|A| |Wq|^T) |wscale| + 2^-24 |bias|
  (K additions, then the epilogue's multiplication by the fp32 column scale and its addition of the fp32 bias).  It does not: on
  an MI355X correct launches exceeded that term on the fp32-output cases (worst ratio 1.52 at 300 x 320 x 128, 0.68 at K = 256, 0.36
  at K = 384: an error that does not grow with K) while every exact-integer case (`exact_operands`, which needs no bound: every
  partial sum is an integer below 2^24, the same bits in any order and under any rounding) was bit-exact.  How the instruction sums
  its 128 products internally is not in the ISA documents at hand, so its error was MEASURED, the instruction alone, one MFMA per
  wave on this module's operand family against fp64 (tools/probe_mfma_fp8.hip:
  `hipcc --offload-arch=gfx950 -O2 tools/probe_mfma_fp8.hip -o probe_mfma_fp8 && ./probe_mfma_fp8` on an MI355X, 2026-10-19):
  max |d - fp64| = 455.83 (mean 22.6) from c = 0 and 443.84 (mean 20.5) from c = an earlier result, in units of
  2^-24 (|c| + sum |a| |b|), over 2 097 152 dot products each: about 2^-15 of the absolute sum, the loss of products aligned to a
  common exponent and truncated, not of fp32 additions.  E_MFMA is twice the maximum.  One 128-deep step is within
  E_MFMA 2^-24 (|c| + its own sum |a| |b|) <= E_MFMA 2^-24 absacc, and there are K / 128 of them:
      |out32 - acc64| <= (E_MFMA K / 128 + 2) 2^-24 (|A| |Wq|^T) |wscale| + 2^-24 |bias|.
* fp32 + residual (epilogue 1): one more fp32 addition, 2 * 2^-24 |want| on top (as test_gpu_gemm_epilogues.py grants).
* RoPE and the gated MLP: gemm_epi_ref.rope_bound / gated_bound fed with the accumulation bound above.
* stores (`worst_ratio(stored=...)`): None = fp32, nothing on top of e.  "bf16": half a bf16 ulp of the stored value, as
  gemm_epi_ref.worst_ratio.  "e4m3": the kernel clamps to +-448 and rounds to nearest even (pack_fp8x4, csrc/common.h), so `want`
  is clamped first (clamping is a contraction: it never increases |y - want|), and half an e4m3 ulp of the STORED value is granted:
  got = m 2^ex with m in [1/2, 1) lies in the binade [2^(ex-1), 2^ex) whose spacing is 2^(ex-1-3); below the smallest normal 2^-6
  the spacing stays 2^-9, hence 2^(max(ex - 1, -6) - 4), and 2^-10 at got == 0 (what rounds to 0 is at most half the smallest
  subnormal away).  A value that rounds UP into the next binade is stored as its lower edge, whose half ulp is the larger one:
  the grant holds there too.  Checked against torch's own cast in test_gemm_fp8_ref.py (worst |cast(y) - y| / grant exactly 1.0, at
  ties).  A NaN byte (0x7F / 0xFF) decodes to NaN: ratio inf.
* LayerNorm with an fp8 result (`layernorm`): two passes over the row in fp32 registers (csrc/rowwise.hip).
  u = 2^-24.  mean32: d - 1 additions in some order and a division: |mean32 - mean| <= em = (d + 1) u mean|x|.
  Second pass q = sum fma(dlt, dlt, q), dlt = fl(x - mean32).  A constant shift c of the mean changes the mean square of the
  deviations by exactly c^2 (the deviations sum to 0), the rounding of each dlt (relative u), of each fma and of the d - 1 wave
  additions and the division by d add (d + 4) u: |var32 - var| <= ev = em^2 + (d + 4) u (var + em^2).
  rstd32 = rsqrtf(var32 + 1e-5): the addition, and rsqrtf itself, taken as 4 ulp: relative er = ev / (2 (var + eps)) + 6 u.
  y = fma((x - mean32) rstd32, gamma, beta): with t = (x - mean) rstd,
      |y32 - y| <= |gamma| (em rstd + |t| (er + 2 u)) + u |y|,
  the 2 u for the subtraction and the multiplication, the last term for the fma's one rounding.  Then the e4m3 store.
  (For a constant row var = 0 and the kernel sees only the rounding of its own mean, amplified by rstd = 316: em rstd |gamma|.)
* row quantiser (`quantize_rows` restates it, `quantize_bound`): scale = amax / 448 (one fp32 division: within one fp32 ulp of the fp64
  quotient), inv = 1 / scale, byte = e4m3(x inv).  Against x itself: |deq scale - x| <= scale (half an e4m3 ulp of deq +
  3 u |x / scale|): inv, the product, and the scale's own rounding folded into the comparison.
"""
import math

import torch

import gemm_epi_ref as E
from gemm_epi_ref import G, ulp32, rope, rope_bound, gated, gated_bound, dtheta_table_free  # noqa: F401  (one copy of each)

E_MFMA = 912.0         # twice the measured 455.83, per 128-deep step, in units of 2^-24 (|c| + sum |a| |b|) (module docstring)
ACC_EXTRA = 2          # the epilogue's roundings: the column scale, the bias
E4M3_MAX = 448.0
LN_EPS = 1e-5
E_RSQRT_ULPS = 4


def deq(u8):
    """e4m3 bytes -> fp64 values (NaN bytes stay NaN)"""
    return u8.view(torch.float8_e4m3fn).float().double()


def to_e4m3(x32):
    """fp32 -> e4m3 bytes, saturating at +-448, RNE: what pack_fp8x4 does"""
    return x32.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def half_ulp_e4m3(got):
    """half the e4m3 spacing at the stored value `got` (fp64), 2^-10 at 0"""
    _, ex = torch.frexp(got)
    h = torch.ldexp(torch.ones_like(got), (ex - 1).clamp_min(-6) - 4)
    return torch.where(got == 0, torch.full_like(got, 2.0 ** -10), h)


def worst_ratio(got, want, e, stored=None):
    """max |got - want| / e over every element (inf where got is not finite, 0 for no element).  stored: None (fp32 output),
    "bf16" or "e4m3" (got = the decoded bytes): half an ulp of the stored value is granted on top of e, and for "e4m3" want is
    clamped to +-448 first."""
    if got.numel() == 0:
        return 0.0
    if stored == "bf16":
        return E.worst_ratio(got, want, e, stored_bf16=True)
    g = got.double()
    if stored == "e4m3":
        want = want.clamp(-E4M3_MAX, E4M3_MAX)
    else:
        assert stored is None, stored
    d = (g - want).abs()
    if stored == "e4m3":
        d = (d - half_ulp_e4m3(torch.where(torch.isfinite(g), g, torch.ones_like(g)))).clamp_min(0.0)
    d = d / e
    d = torch.where(torch.isfinite(g), d, torch.full_like(d, math.inf))
    return float(d.max())


# ------------------------------------------------------------------ data ------------------------------------------------------------------
def row_factors(n, seed):
    """n factors spread geometrically over 0.01 .. 30 in a fixed shuffled order: neighbours differ by decades"""
    f = torch.logspace(-2, math.log10(30.0), n, dtype=torch.float64) if n > 1 else torch.ones(1, dtype=torch.float64)
    return f[torch.randperm(n, generator=torch.Generator().manual_seed(1000 + seed))].float()


def quantize_rows(w):
    """pack_fp8_kernel in torch: (bytes [rows, cols], scales fp32 [rows])"""
    w = w.float()
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    inv = 1.0 / scale
    return to_e4m3(w * inv[:, None]), scale


HOT_PAIRS = 6      # fc1 / gate column pairs of the gated data scaled 600: outputs beyond +-448


def weights(N, K, seed, gated_data=False):
    """fp32 [N, K] weights and [N] bias before quantisation: asym / sqrt(K) (0.1 asym) times a per-row factor over three decades; the
    gated family gets a few packed (fc1 row, gate row) pairs at factor 600"""
    from gpu_util import asym
    fw, fb = row_factors(N, seed), row_factors(N, seed + 7)
    if gated_data:
        hot = torch.randperm(N // 32, generator=torch.Generator().manual_seed(seed))[:HOT_PAIRS] * 32 + 5
        fw[hot], fw[hot + 16] = 600.0, 600.0
    W = asym((N, K), seed + 1) / math.sqrt(K) * fw[:, None]
    b = 0.1 * asym((N,), seed + 2) * fb
    return W.float().contiguous(), b.float().contiguous()


def operands(M, N, K, seed, device="cpu", quant=quantize_rows, gated_data=False):
    """(A bytes [M, K], Wq bytes [N, K], wscale fp32 [N], bias fp32 [N]) on `device`; quant: fp32 [N, K] on the device -> (bytes,
    scales) (the GPU tests pass ditto_quantize_rows_fp8, the CPU tests the torch restatement above)"""
    from gpu_util import asym
    A = asym((M, K), seed).float().to(torch.float8_e4m3fn).view(torch.uint8).to(device)
    W, b = weights(N, K, seed, gated_data)
    Wq, ws = quant(W.to(device))
    return A, Wq, ws, b.to(device)


def exact_operands(M, N, K, seed, device="cpu"):
    """integers: A in [-3, 3], W in [-2, 2] (as e4m3 bytes), wscale 2^((n mod 7) - 3), bias multiples of 2^-4 in [-4, 4]: every
    partial sum, the scaled sum and the biased sum are exactly representable in fp32"""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-2, 3, (N, K), generator=g).float()
    ws = torch.ldexp(torch.ones(N), (torch.arange(N) % 7 - 3).int()).float()
    b = torch.randint(-64, 65, (N,), generator=g).float() / 16
    return to_e4m3(A).to(device), to_e4m3(W).to(device), ws.to(device), b.to(device)


def e4m3_edges(want):
    """(elements beyond +-448, elements in the e4m3 subnormal range [2^-10, 2^-6)) of a reference: both edges of the format"""
    a = want.abs()
    return int((a > E4M3_MAX).sum()), int(((a >= 2.0 ** -10) & (a < 2.0 ** -6)).sum())


def layernorm_data(M, d, seed):
    """x fp32 [M + 1, d] = asym * 1.7 + 0.3 with a constant last row (variance 0); gamma with every eighth column scaled 400 (those
    outputs saturate wherever |t| > 1.12); beta"""
    from gpu_util import asym
    x = (asym((M + 1, d), seed) * 1.7 + 0.3).float()
    x[-1] = 1.7
    g = (1 + 0.1 * asym((d,), seed + 1)).float()
    g[3::8] *= 400.0
    return x.contiguous(), g.contiguous(), (0.1 * asym((d,), seed + 2)).float().contiguous()


def quantize_data(rows, cols, seed):
    """fp32 [rows, cols]: rows scaled over three decades; from 5 rows on, row 1 is all zero, row 2 has its maximum negative and in
    the last column, row 3 has one element 1e4 times the rest (the rest land in e4m3 subnormals and zero)"""
    from gpu_util import asym
    x = (asym((rows, cols), seed) * row_factors(rows, seed)[:, None]).float()
    if rows >= 5:
        x[1] = 0.0
        x[2, -1] = -2.0 * float(x[2].abs().max())
        x[3, 1] = 1e4 * float(x[3].abs().max())
    return x.contiguous()


# --------------------------------------------------------------- references ---------------------------------------------------------------
def linear(Aq, Wq, wscale=None, bias=None):
    """acc64 = (A Wq^T) wscale + bias and its accumulation bound (both [M, N] fp64) from the bytes"""
    A, W = deq(Aq), deq(Wq)
    K = A.shape[1]
    acc, absacc = A @ W.T, A.abs() @ W.abs().T
    if wscale is not None:
        acc, absacc = acc * wscale.double(), absacc * wscale.double().abs()
    bound = (E_MFMA * (K // 128) + ACC_EXTRA) * G * absacc
    if bias is not None:
        acc, bound = acc + bias.double(), bound + G * bias.double().abs()
    return acc, bound + 1e-30


def layernorm_terms(x):
    """(t, rstd, em, er) of the module docstring for rows x: t = (x - mean) rstd in fp64, rstd [rows, 1], em the bound on the fp32
    mean, er the relative bound on the fp32 rstd (gemm_fr_ref.py propagates a row perturbation through the same terms)"""
    x = x.double()
    d = x.shape[1]
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    t = (x - mean) * rstd
    em = (d + 1) * G * x.abs().mean(dim=1, keepdim=True)
    ev = em * em + (d + 4) * G * (var + em * em)
    er = ev / (2 * (var + LN_EPS)) + (2 + E_RSQRT_ULPS) * G
    return t, rstd, em, er


def layernorm(x, gamma=None, beta=None):
    """fp64 LayerNorm (biased variance, eps 1e-5) of fp32 rows and the bound of the module docstring, before the e4m3 store"""
    t, rstd, em, er = layernorm_terms(x)
    d = x.shape[1]
    g = gamma.double() if gamma is not None else torch.ones(d, dtype=torch.float64, device=x.device)
    y = t * g + (beta.double() if beta is not None else 0.0)
    return y, g.abs() * (em * rstd + t.abs() * (er + 2 * G)) + G * y.abs() + 1e-30


def quantize_bound(x, q, scales):
    """(|deq scale - x|, its bound) elementwise for fp32 rows x, bytes q and fp32 scales (module docstring)"""
    s = scales.double()[:, None]
    dq = deq(q)
    return (dq * s - x.double()).abs(), s * (half_ulp_e4m3(torch.where(torch.isfinite(dq), dq, torch.ones_like(dq))) + 3 * G * (x.double() / s).abs())
