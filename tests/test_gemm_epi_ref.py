"""Keeps tests/gemm_epi_ref.py honest without a GPU: the fp64 references against independent statements of the same formulas (the
oracle's apply_rope, torch's gelu / sigmoid, fp64 autograd), and the BOUNDS against a correct fp32 evaluation of every operation
on every input family test_gpu_gemm_epilogues.py uses (fp32 matmul on the bf16 operands + the fp32 formula + bf16 rounding):
worst_ratio <= 1, so each bound is shown to admit a right implementation before it meets the kernel.  -s prints the ratios."""
import math

import pytest
import torch

import gemm_epi_ref as R
from oracle import ditto_oracle as O


def test_rope_is_the_oracles_apply_rope():
    """G1-sized: 64 rows, 4 heads of 64 (hidden 256), q and k rotated, v not"""
    g = torch.Generator().manual_seed(3)
    n, H = 64, 4
    q, k, v = (torch.randn(1, n, H, 64, dtype=torch.float64, generator=g) for _ in range(3))
    invf = O.rotary_inv_freq(64)
    assert torch.equal(invf, R.inv_freq(64))
    tab = O.rotary_table(invf.double(), n)
    want = torch.cat([O.apply_rope(tab, q).reshape(n, -1), O.apply_rope(tab, k).reshape(n, -1), v.reshape(n, -1)], dim=1)
    pre = torch.cat([q.reshape(n, -1), k.reshape(n, -1), v.reshape(n, -1)], dim=1)
    pos = torch.arange(n)
    c, s = R.rope_exact_tables(invf, pos)
    got = R.rope(pre, pos, 2 * H * 64, c, s)
    assert float((got - want).abs().max()) < 1e-13
    assert torch.equal(got[:, 2 * H * 64:], pre[:, 2 * H * 64:])
    # the fp32 tables differ from the exact angles by fp32 rounding only
    ct, st = R.tables(invf, n)
    assert float((R.rope(pre, pos, 2 * H * 64, ct, st) - want).abs().max()) < 1e-6


def test_interleave_helpers_are_inverses():
    x = torch.arange(3 * 96, dtype=torch.float64).reshape(3, 96)
    a, g = R.deinterleave(x)
    assert a.shape == g.shape == (3, 48)
    assert torch.equal(a[0, :16], x[0, :16]) and torch.equal(g[0, :16], x[0, 16:32]) and torch.equal(a[0, 16:32], x[0, 32:48])
    assert torch.equal(R.interleave(a, g), x)
    a2, g2 = R.deinterleave(R.interleave(g, a))
    assert torch.equal(a2, g) and torch.equal(g2, a)


def test_gated_is_gelu_times_sigmoid_and_its_backward_is_autograd():
    g = torch.Generator().manual_seed(5)
    pre = (2.5 * torch.randn(37, 128, dtype=torch.float64, generator=g)).requires_grad_(True)
    a, gt = R.deinterleave(pre)
    want = torch.nn.functional.gelu(a) * torch.sigmoid(gt)
    y = R.gated(pre)
    assert float((y - want).abs().max()) < 1e-14
    dact = torch.randn(37, 64, dtype=torch.float64, generator=g)
    (grad,) = torch.autograd.grad(want, pre, dact)
    got = R.gated_bwd(dact, pre.detach())
    assert float((got - grad).abs().max()) < 1e-13
    # the derivative magnitudes gated_bound relies on
    x = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    assert float((R._Phi(x) + x * R._phi(x)).abs().max()) <= 1.13


def test_colsum_partials_rows():
    x = torch.ones(300, 4, dtype=torch.float64)
    s, sa = R.colsum_partials(x, 300)
    assert s.shape == (4, 4) and s[:, 0].tolist() == [128.0, 128.0, 44.0, 0.0] and torch.equal(s, sa)


def test_ulp32_and_the_angle_bound():
    x = torch.tensor([1.0, 1.5, 2.0, 651.7, 0.0], dtype=torch.float64)
    assert R.ulp32(x).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -14, 0.0]
    d = R.dtheta_table_free(torch.tensor([4095]), R.inv_freq())
    assert 3.5e-4 < float(d[0, 0]) < 4.5e-4        # pos 4095, j = 0: both terms, not the 2e-4 of the first alone
    assert float(R.dtheta_table_free(torch.tensor([0]), R.inv_freq()).max()) == 0.0
    # and it does bound the fp32 evaluation of the angle
    pos = torch.arange(4096)
    f = R.freq_rev(R.inv_freq())
    t = pos.float()[:, None] * f[None, :]
    rev = (t - t.floor()).double()
    exact = pos.double()[:, None] * R.inv_freq().double()[None, :] / (2 * math.pi)
    err = (rev - exact + 0.5).remainder(1.0) - 0.5           # wrapped to [-1/2, 1/2)
    assert bool((2 * math.pi * err.abs() <= R.dtheta_table_free(pos, R.inv_freq()) + 1e-15).all())


# ------------------------------------------------ fp32 evaluation of every GPU input family ------------------------------------------------
def _acc32(A, W, b):
    acc = A.float() @ W.float().T
    return acc + b if b is not None else acc


def _rope32(acc, pos, rope_cols, cs, sn):
    lo, hi = R._split(acc, rope_cols)
    c, s = cs[pos][:, None, :], sn[pos][:, None, :]
    return R._join(lo * c - hi * s, hi * c + lo * s, acc[:, rope_cols:])


@pytest.mark.parametrize("rpb,M,d,K", [(1024, 2048, 256, 256), (200, 1000, 320, 320), (4096, 4396, 128, 128), (333, 999, 256, 64)])
@pytest.mark.parametrize("table_free", [True, False])
def test_fp32_rope_sits_inside_the_bound(rpb, M, d, K, table_free):
    N, rc = 3 * d, 2 * d
    A, W, b = R.operands(M, N, K, 11)
    pre, absacc = R.linear(A, W, b)
    accb = R.acc_bound(absacc, K)
    invf = R.inv_freq()
    pos = torch.arange(M) % rpb
    if table_free:
        f = R.freq_rev(invf)
        t = pos.float()[:, None] * f[None, :]
        rev = (t - t.floor()).double() * 2 * math.pi
        cs, sn = rev.cos().float(), rev.sin().float()          # a correctly rounded v_cos / v_sin
        got = _rope32(_acc32(A, W, b), torch.arange(M), rc, cs, sn)
        c64, s64 = R.rope_exact_tables(invf, pos)
        want = R.rope(pre, torch.arange(M), rc, c64, s64)
        bound = R.rope_bound(pre, accb, rc, R.dtheta_table_free(pos, invf), R.E_SINCOS)
    else:
        cs, sn = R.tables(invf, rpb)
        got = _rope32(_acc32(A, W, b), pos, rc, cs, sn)
        want = R.rope(pre, pos, rc, cs, sn)
        bound = R.rope_bound(pre, accb, rc)
    r = R.worst_ratio(got.to(torch.bfloat16), want, bound, stored_bf16=True)
    print(f"rope rpb {rpb} M {M} d {d} K {K} table_free {table_free}: worst ratio {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("M,N,K", [(300, 320, 192), (513, 2336, 64), (777, 1024, 768)])
def test_fp32_gated_and_plain_epilogues_sit_inside_the_bound(M, N, K):
    A, W, b = R.operands(M, N, K, 21)
    pre, absacc = R.linear(A, W, b)
    accb = R.acc_bound(absacc, K)
    acc = _acc32(A, W, b)
    out = {}
    out["bias_bf16"] = R.worst_ratio(acc.to(torch.bfloat16), pre, accb, stored_bf16=True)
    out["relu_bf16"] = R.worst_ratio(acc.clamp_min(0).to(torch.bfloat16), pre.clamp_min(0), accb, stored_bf16=True)
    out["bias_f32"] = R.worst_ratio(acc, pre, accb)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(1))
    out["bias_res_f32"] = R.worst_ratio(acc + res, pre + res.double(), accb + R.G * (pre + res.double()).abs())
    a32, g32 = R.deinterleave(acc)
    y = torch.nn.functional.gelu(a32) * torch.sigmoid(g32)
    out["gated"] = R.worst_ratio(y.to(torch.bfloat16), R.gated(pre), R.gated_bound(pre, accb), stored_bf16=True)
    out["gated_pre"] = R.worst_ratio(acc.to(torch.bfloat16), pre, accb, stored_bf16=True)
    print(f"M {M} N {N} K {K}: " + "  ".join(f"{k} {v:.3f}" for k, v in out.items()))
    assert max(out.values()) <= 1.0, out


@pytest.mark.parametrize("M,F,K", [(300, 256, 768), (513, 512, 64)])
def test_fp32_gated_backward_sits_inside_the_bound(M, F, K):
    from gpu_util import asym
    A, W, _ = R.operands(M, F, K, 41, bias=False)
    pre = (1.5 * asym((M, 2 * F), 44)).to(torch.bfloat16)
    dact, absacc = R.linear(A, W)
    accb = R.acc_bound(absacc, K)
    dy = _acc32(A, W, None).to(torch.bfloat16).float()
    a, g = R.deinterleave(pre.float())
    sg = torch.sigmoid(g)
    Phi = 0.5 * (1 + torch.erf(a * 0.7071067811865476))
    phi = torch.exp(-0.5 * a * a) * 0.3989422804014327
    got = R.interleave(dy * sg * (Phi + a * phi), dy * sg * (a * Phi) * (1 - sg)).to(torch.bfloat16)
    r = R.worst_ratio(got, R.gated_bwd(dact, pre), R.gated_bwd_bound(dact, accb, pre), stored_bf16=True)
    print(f"gated_bwd M {M} F {F} K {K}: worst ratio {r:.3f}")
    assert r <= 1.0
