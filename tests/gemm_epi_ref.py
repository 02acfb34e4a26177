"""fp64 references and elementwise error bounds for the bf16 GEMM family's fused epilogues (csrc/gemm_common.h), shared by
test_gemm_epi_ref.py (no GPU) and test_gpu_gemm_epilogues.py.  Plain torch on the bf16-rounded operands the kernel saw; every
function returns the expected value AND a bound on |kernel - expected| derived from the kernel's arithmetic, never a fitted
constant.  The terms:

* accumulation: the MFMA sums K products of bf16 values (exact in fp32) in fp32, in some order, and the epilogue adds the fp32
  bias: |acc32 - acc64| <= (K + 1) 2^-24 absacc, absacc = |A| |W|^T + |bias|          (`linear`, `acc_bound`).
* RoPE (`rope`, `rope_bound`): out_lo = lo cos - hi sin, out_hi = hi cos + lo sin on the pair (j, j + 32) of a 64-wide head.
  Both partners' accumulation bounds (|cos|, |sin| <= 1), an angle error dtheta moves the output by <= dtheta hypot(lo, hi), an
  error e on the sin / cos VALUES by <= e (|lo| + |hi|), the three fp32 operations of the rotation by 3 * 2^-24 (|lo| + |hi|).
  Table-free angles (`dtheta_table_free`): the kernel forms rev = fract(fp32(pos * f)), f = fp32(inv_freq / (2 pi)): f is off
  by <= ulp32(f) / 2 and the product by <= ulp32(pos f) / 2, fract is exact, so dtheta = 2 pi (ulp32(pos f) / 2 + pos ulp32(f) / 2)
  (3.8e-4 rad at pos 4095, j = 0).  The error of v_sin_f32 / v_cos_f32 themselves is not in the ISA documents at hand and was
  MEASURED, the instructions alone against fp64 sin / cos of 2 pi times the same fp32 argument (tools/probe_sincos.hip:
  `hipcc --offload-arch=gfx950 -O2 tools/probe_sincos.hip -o probe_sincos && ./probe_sincos` on an MI355X): max |v_sin - sin|
  1.199e-07 and max |v_cos - cos| 1.237e-07 over the 4096 x 32 arguments of the epilogue, 1.237e-07 for both over [0, 1) in
  steps of 2^-20.  E_SINCOS is twice the maximum.  Table path: the reference reads the same fp32 tables: dtheta = 0, e = 0.
* gated MLP (`gated`, `gated_bound`): y = gelu_erf(a) sigmoid(g); |dy/da| <= 1.13, |dy/dg| <= |gelu(a)| / 4, so the accumulation
  bounds propagate as 1.13 ba + (|gelu(a)| + 1.13 ba) bg / 4; the kernel's rational erf adds what tests/test_gated_math.py pins
  for the product as evaluated in fp32: 3e-6 absolute on |a| <= 12 (5e-4 relative beyond, where that test's sweep is relative).
* gated backward (`gated_bwd`, `gated_bwd_bound`): the kernel rounds dact to bf16 first (relative 2^-8 of a value within its
  accumulation bound), then multiplies by ca = sigmoid(g) (Phi(a) + a phi(a)) or cg = gelu(a) sigmoid(g) (1 - sigmoid(g)) computed
  in fp32 from the rational erf (6e-7 on erf: 3e-7 on Phi), one v_exp and two v_rcp (an ulp or two each) and a handful of fp32
  operations: each coefficient within 2e-6 (1 + |a|).
* a bf16 store rounds to nearest: half an ulp of the stored value, granted by `worst_ratio(stored_bf16=True)` exactly as
  attn_ref.worst_ratio does (bf16 has 8 significant bits: up to 2^-8 of the value just above a power of two, so a flat 2^-9 |want|
  would refuse correctly rounded results).
"""
import math

import torch

G = 2.0 ** -24          # fp32 unit roundoff
E_SINCOS = 2.5e-7       # twice the measured 1.237e-07 (module docstring)
GATED_ABS, GATED_REL = 3e-6, 5e-4   # tests/test_gated_math.py


def worst_ratio(got, want, e, stored_bf16=False):
    """max |got - want| / e over every element (inf where got is not finite, 0 for no element).  stored_bf16: got is the bf16
    rounding of a value within e of want: half a bf16 ulp of got is granted on top of e."""
    if got.numel() == 0:
        return 0.0
    g = got.double()
    d = (g - want).abs()
    if stored_bf16:
        _, ex = torch.frexp(g)
        d = (d - torch.ldexp(torch.ones_like(g), ex - 9)).clamp_min(0.0)
    d = d / e
    d = torch.where(torch.isfinite(g), d, torch.full_like(d, math.inf))
    return float(d.max())


def ulp32(x):
    """spacing of fp32 numbers at |x| (fp64 tensor in the normal range; 0 at 0)"""
    _, ex = torch.frexp(x.double().abs())
    return torch.where(x == 0, torch.zeros_like(x, dtype=torch.float64), torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex - 24))


def operands(M, N, K, seed, device="cpu", bias=True):
    """the input family of every GPU test: asymmetric sign-varying A, weights scaled 1 / sqrt(K), bias 0.1 * asym"""
    from gpu_util import asym
    A = asym((M, K), seed).to(torch.bfloat16).to(device)
    W = (asym((N, K), seed + 1) / math.sqrt(K)).to(torch.bfloat16).to(device)
    b = (0.1 * asym((N,), seed + 2)).float().to(device) if bias else None
    return A, W, b


def linear(A, W, bias=None):
    """acc64 = A W^T + bias in fp64 and absacc = |A| |W|^T + |bias| (both [M, N])"""
    A64, W64 = A.double(), W.double()
    acc, absacc = A64 @ W64.T, A64.abs() @ W64.abs().T
    if bias is not None:
        acc, absacc = acc + bias.double(), absacc + bias.double().abs()
    return acc, absacc


def acc_bound(absacc, K):
    return (K + 1) * G * absacc + 1e-30


# ------------------------------------------------------------------ RoPE ------------------------------------------------------------------
def inv_freq(head_dim=64):
    """fp32 [head_dim / 2], as the model's rotary.inv_freq (reference src/components/DiT.py:49)"""
    return 1.0 / (10000 ** (torch.arange(0, head_dim, 2).float() / head_dim))


def freq_rev(invf):
    """what the kernel is given for the table-free angles: fp32(inv_freq / (2 pi))"""
    return (invf.double() / (2 * math.pi)).float()


def tables(invf, positions):
    """fp32 cos / sin [positions, 32] of pos * inv_freq evaluated in fp64 (the table path reads these)"""
    th = torch.arange(positions, dtype=torch.float64, device=invf.device)[:, None] * invf.double()[None, :]
    return th.cos().float().contiguous(), th.sin().float().contiguous()


def dtheta_table_free(pos, invf):
    """[M, 32] bound (radians) on the kernel's angle against pos * inv_freq: see the module docstring"""
    f = freq_rev(invf).double()
    p = pos.double()[:, None]
    return 2 * math.pi * (ulp32(p * f[None, :]) / 2 + p * ulp32(f)[None, :] / 2)


def _split(x, rope_cols):
    M = x.shape[0]
    h = x[:, :rope_cols].reshape(M, rope_cols // 64, 2, 32)
    return h[:, :, 0], h[:, :, 1]


def _join(lo, hi, rest):
    M = lo.shape[0]
    return torch.cat([torch.stack([lo, hi], dim=2).reshape(M, -1), rest], dim=1)


def rope(pre, pos, rope_cols, cos, sin):
    """pre [M, N] = acc + bias; columns < rope_cols rotated per 64-wide head at angle (cos, sin)[pos] ([M, 32] each after the
    gather), identity beyond.  cos / sin: [positions, 32] tables (any float type; used in fp64)."""
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    lo, hi = _split(pre, rope_cols)
    return _join(lo * c - hi * s, hi * c + lo * s, pre[:, rope_cols:])


def rope_exact_tables(invf, pos):
    """fp64 cos / sin [M, 32] at pos * inv_freq (index with arange(M))"""
    th = pos.double()[:, None] * invf.double()[None, :]
    return th.cos(), th.sin()


def rope_bound(pre, accb, rope_cols, dtheta=None, e_sincos=0.0):
    """elementwise bound before the bf16 store.  dtheta: [M, 32] or None (table path: 0)"""
    lo, hi = _split(pre, rope_cols)
    blo, bhi = _split(accb, rope_cols)
    mag = lo.abs() + hi.abs()
    b = blo + bhi + (e_sincos + 3 * G) * mag
    if dtheta is not None:
        b = b + dtheta[:, None, :] * torch.hypot(lo, hi)
    return _join(b, b, accb[:, rope_cols:]) + 1e-30


# --------------------------------------------------------------- gated MLP ---------------------------------------------------------------
def deinterleave(x):
    """packed columns [16 x fc1 | 16 x gate | ...] -> (a, g), each [..., N / 2]"""
    s = x.shape
    h = x.reshape(*s[:-1], s[-1] // 32, 2, 16)
    return h[..., 0, :].reshape(*s[:-1], s[-1] // 2), h[..., 1, :].reshape(*s[:-1], s[-1] // 2)


def interleave(a, g):
    s = a.shape
    return torch.stack([a.reshape(*s[:-1], s[-1] // 16, 16), g.reshape(*s[:-1], s[-1] // 16, 16)], dim=-2).reshape(*s[:-1], 2 * s[-1])


def _phi(a):
    return torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)


def _Phi(a):
    return 0.5 * (1 + torch.erf(a / math.sqrt(2)))


def gated(pre):
    """pre [M, N] packed -> gelu_erf(a) * sigmoid(g) [M, N / 2] (reference src/components/DiT.py:153-155)"""
    a, g = deinterleave(pre)
    return a * _Phi(a) * torch.sigmoid(g)


def gated_bound(pre, accb):
    a, g = deinterleave(pre)
    ba, bg = deinterleave(accb)
    gelu = (a * _Phi(a)).abs()
    want = gelu * torch.sigmoid(g)
    erf_term = torch.where(a.abs() <= 12, torch.full_like(want, GATED_ABS), GATED_ABS + GATED_REL * want)
    return 1.13 * ba + (gelu + 1.13 * ba) * bg / 4 + erf_term


def gated_bwd(dact, pre):
    """dact [M, F] fp64, pre [M, 2F] packed (the bf16 values the kernel reads) -> [da | dg] packed [M, 2F] fp64"""
    a, g = deinterleave(pre.double())
    sg = torch.sigmoid(g)
    ca = sg * (_Phi(a) + a * _phi(a))
    cg = a * _Phi(a) * sg * (1 - sg)
    return interleave(dact * ca, dact * cg)


def gated_bwd_bound(dact, accb, pre):
    a, g = deinterleave(pre.double())
    sg = torch.sigmoid(g)
    ca = (sg * (_Phi(a) + a * _phi(a))).abs()
    cg = (a * _Phi(a) * sg * (1 - sg)).abs()
    ddy = accb + 2.0 ** -8 * (dact.abs() + accb)      # dact in fp32, then rounded to bf16
    ec = 2e-6 * (1 + a.abs())
    dy = dact.abs() + ddy
    return interleave(ca * ddy + dy * ec, cg * ddy + dy * ec) + 1e-30


def colsum_partials(x, M):
    """x [M, C] -> (sums, abs sums) fp64 [2 * ceil(M / 256), C]: one row per 128 rows, rows past M contribute nothing
    (csrc/kernels.h colsum_partial)"""
    rows = 2 * ((M + 255) // 256)
    x = x.double()
    pad = torch.zeros(rows * 128 - M, x.shape[1], dtype=torch.float64, device=x.device)
    xp = torch.cat([x, pad]).reshape(rows, 128, x.shape[1])
    return xp.sum(1), xp.abs().sum(1)
