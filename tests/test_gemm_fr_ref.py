"""gemm_fr_ref.py without a GPU: a plain torch fp32 imitation of each full-row kernel (blocked matmul in another order from
fl32(residual + bias), then a two-pass fp32 LayerNorm) sits inside its bound, and every mutation of that imitation that a wrong
kernel could be (a wrong eps, an unbiased variance, statistics over half a row, an affine vector read one 256-column piece or one
wave's width off, the next row's residual, the LayerNorm of the rounded row, a K slab dropped or counted twice, a second rounding)
leaves it: the evidence that test_gpu_gemm_fr.py would notice."""
import pytest
import torch

import gemm_fr_ref as R
from gemm_fp8_ref import to_e4m3

M = 16


def bf(x):
    return x.to(torch.bfloat16)


def imit_h(c, rot=0, drop=None, twice=None, res_next=False, bias_rot=0, res=True, bias=True):
    """fp32 accumulators from fl32(residual + bias), then the K slabs of 16 from slab `rot` on, wrapping"""
    A, W = c["A"].float(), c["W"].float()
    acc = torch.zeros(A.shape[0], W.shape[0])
    if res:
        acc = acc + (torch.roll(c["res"], -1, 0) if res_next else c["res"])
    if bias:
        acc = acc + torch.roll(c["bias"], bias_rot)
    ns = A.shape[1] // 16
    for i in range(ns):
        s = (rot + i) % ns
        if s == drop:
            continue
        for _ in range(2 if s == twice else 1):
            acc = acc + A[:, 16 * s:16 * s + 16] @ W[:, 16 * s:16 * s + 16].T
    return acc


def imit_ln(x, gamma, beta, eps=1e-5, unbiased=False, half=False, g_rot=0, b_rot=0):
    """two passes in fp32, as nn.LayerNorm"""
    x = x.float()
    d = x.shape[1]
    xs = x[:, :d // 2] if half else x
    n = xs.shape[1]
    mean = xs.sum(dim=1, keepdim=True) / n
    dl = xs - mean
    var = (dl * dl).sum(dim=1, keepdim=True) / (n - 1 if unbiased else n)
    rstd = torch.rsqrt(var + eps)
    return (x - mean) * rstd * torch.roll(gamma, g_rot) + torch.roll(beta, b_rot)


LN_MUTATIONS = [dict(eps=1e-6), dict(unbiased=True), dict(half=True)]
WAVE = {768: 192, 1024: 256}


def vec_mutations(N):
    return [{k: s} for k in ("g_rot", "b_rot") for s in (256, WAVE[N])]


H_MUTATIONS = [dict(res_next=True), dict(drop=1), dict(twice=2)]


# ------------------------------------------------------------- the fp32 stream -------------------------------------------------------------
def f32_ratios(c, K, h, u, stored="bf16"):
    h64, hb = R.h_ref(c["A"], c["W"], c["bias"], c["res"])
    want, e = R.layernorm(h, c["gamma"], c["beta"])                     # of the h the (imitated) kernel stored
    got = u.float() if stored == "bf16" else R.deq(u)
    return R.worst_ratio(h, h64, hb), R.worst_ratio(got, want, e, stored=stored)


@pytest.mark.parametrize("N,K", [(768, 64), (768, 768), (1024, 64), (1024, 256)])
def test_fp32_stream_imitation_sits_inside_the_bound_and_the_bugs_do_not(N, K):
    c = R.case(M, N, K, 11)
    g, b = c["gamma"], c["beta"]
    for rot in (0, 1, K // 32):
        h = imit_h(c, rot=rot)
        rh, ru = f32_ratios(c, K, h, bf(imit_ln(h, g, b)))
        print(f"N{N} K{K} rot{rot}: h {rh:.3f} u {ru:.3f}")
        assert rh <= 1 and ru <= 1, (rot, rh, ru)
    h = imit_h(c)
    for mut in LN_MUTATIONS + vec_mutations(N):
        _, ru = f32_ratios(c, K, h, bf(imit_ln(h, g, b, **mut)))
        assert ru > 1, (mut, ru)
    _, ru = f32_ratios(c, K, h, bf(imit_ln(bf(h), g, b)))               # the LayerNorm of the bf16-rounded row
    assert ru > 1, ru
    for mut in H_MUTATIONS + [dict(bias_rot=256), dict(bias_rot=WAVE[N])]:
        hm = imit_h(c, **mut)
        rh, _ = f32_ratios(c, K, hm, bf(imit_ln(hm, g, b)))
        assert rh > 1, (mut, rh)


def test_fp32_stream_without_residual_or_bias():
    N, K = 768, 128
    c = R.case(M, N, K, 12)
    for res, bias in ((False, True), (True, False), (False, False)):
        h = imit_h(c, res=res, bias=bias)
        h64, hb = R.h_ref(c["A"], c["W"], c["bias"] if bias else None, c["res"] if res else None)
        assert R.worst_ratio(h, h64, hb) <= 1
        assert R.worst_ratio(imit_h(c, res=res, bias=bias, drop=0), h64, hb) > 1


def test_fp8_u_imitation_reaches_both_edges_of_e4m3():
    N, K = 1024, 64
    c = R.case(M, N, K, 13, gscale=16.0)
    g, b = c["gamma"], c["beta"]
    h = imit_h(c)
    want, _ = R.layernorm(h, g, b)
    sat, sub = R.e4m3_edges(want)
    assert sat >= 32 and sub >= 32, (sat, sub)
    rh, ru = f32_ratios(c, K, h, to_e4m3(imit_ln(h, g, b)), stored="e4m3")
    assert rh <= 1 and ru <= 1, (rh, ru)
    for mut in LN_MUTATIONS + vec_mutations(N):
        _, ru = f32_ratios(c, K, h, to_e4m3(imit_ln(h, g, b, **mut)), stored="e4m3")
        assert ru > 1, (mut, ru)


# ------------------------------------------------------------- the bf16 stream -------------------------------------------------------------
def hb_ratios(c, h16, u):
    h64, hb = R.h_ref(c["A"], c["W"], c["bias"], c["res"])
    want, e = R.layernorm_of_perturbed(h64, hb, c["gamma"], c["beta"])
    return R.worst_ratio(h16.float(), h64, hb, stored="bf16"), R.worst_ratio(u.float(), want, e, stored="bf16")


@pytest.mark.parametrize("K", [64, 768])
def test_bf16_stream_imitation_sits_inside_the_bound_and_the_bugs_do_not(K):
    N = 768
    c = R.case(M, N, K, 14, stream="bf16")
    g, b = c["gamma"], c["beta"]
    assert torch.equal(c["res"], bf(c["res"]).float())
    for rot in (0, K // 32):
        h = imit_h(c, rot=rot)
        rh, ru = hb_ratios(c, bf(h), bf(imit_ln(h, g, b)))              # the UNROUNDED row is normalised
        print(f"hb K{K} rot{rot}: h {rh:.3f} u {ru:.3f}")
        assert rh <= 1 and ru <= 1, (rot, rh, ru)
    h = imit_h(c)
    for mut in LN_MUTATIONS + vec_mutations(N):
        _, ru = hb_ratios(c, bf(h), bf(imit_ln(h, g, b, **mut)))
        assert ru > 1, (mut, ru)
    _, ru = hb_ratios(c, bf(h), bf(imit_ln(bf(h), g, b)))               # the LayerNorm of the STORED row: not what the kernel does
    assert ru > 1, ru
    for mut in H_MUTATIONS + [dict(bias_rot=256), dict(bias_rot=192)]:
        hm = imit_h(c, **mut)
        rh, _ = hb_ratios(c, bf(hm), bf(imit_ln(hm, g, b)))
        assert rh > 1, (mut, rh)


def test_perturbation_bound_covers_a_worst_case_row_shift():
    """dx = +-hb with the signs that move the statistics most (along t, and all one way) stays inside the propagated bound without
    any arithmetic error at all: the first-order terms and the remainder are not too small"""
    N, K = 768, 3072
    c = R.case(M, N, K, 15, stream="bf16")
    h64, hb = R.h_ref(c["A"], c["W"], c["bias"], c["res"])
    want, e = R.layernorm_of_perturbed(h64, hb, c["gamma"], c["beta"])
    t = (h64 - h64.mean(1, keepdim=True))
    for sign in (torch.sign(t), -torch.sign(t), torch.ones_like(t), torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0).double()):
        got, _ = R.layernorm(h64 + sign * hb, c["gamma"], c["beta"])
        assert R.worst_ratio(got, want, e) <= 1


# ------------------------------------------------------------------ lnq ------------------------------------------------------------------
def imit_lnq(x, g, b, W, bias, y_round=bf, rot=0, **mut):
    y = y_round(imit_ln(x, g, b, **mut)).float()
    c = dict(A=y, W=W, res=None, bias=bias)
    return bf(imit_h(c, rot=rot, res=False, bias=bias is not None))


def round7(x):
    """a SECOND rounding: to seven significant bits (twice bf16's spacing), ties away"""
    m, ex = torch.frexp(x.float())
    return torch.ldexp(torch.round(m * 128) / 128, ex)


@pytest.mark.parametrize("d", [768, 1024])
@pytest.mark.parametrize("bf16_rows", [False, True])
def test_lnq_imitation_sits_inside_the_bound_and_the_bugs_do_not(d, bf16_rows):
    from gpu_util import asym
    x = R.lnq_rows(M, d, 21, bf16_rows)
    bias, g, b = R.affine(d, 22)
    W = bf(asym((d, d), 23) / d ** 0.5)
    for use_bias in (True, False):
        bb = bias if use_bias else None
        want, e = R.lnq_ref(x, g, b, W, bb)
        for rot in (0, 16):
            r = R.worst_ratio(imit_lnq(x, g, b, W, bb, rot=rot).float(), want, e, stored="bf16")
            print(f"lnq d{d} bias{use_bias} rot{rot}: {r:.3f}")
            assert r <= 1, r
        assert R.worst_ratio(imit_lnq(x, g, b, W, bb, y_round=lambda y: y).float(), want, e, stored="bf16") <= 1   # y left unrounded
        # (an unbiased variance scales every y_k of a row by 1 - 1 / (2 d), far inside the 2^-8 |y_k| each may be off through a general
        # W: it shows through the identity below, where the product adds nothing)
        for mut in [m for m in LN_MUTATIONS if "unbiased" not in m] + vec_mutations(d):
            r = R.worst_ratio(imit_lnq(x, g, b, W, bb, **mut).float(), want, e, stored="bf16")
            assert r > 1, (mut, r)
    want, e = R.lnq_ref(x, g, b, W, bias)
    for rot in (256, d // 4):
        c = dict(A=bf(imit_ln(x, g, b)), W=W, bias=bias, res=None)
        for mut in (dict(bias_rot=rot), dict(drop=3), dict(twice=5)):
            assert R.worst_ratio(bf(imit_h(c, res=False, **mut)).float(), want, e, stored="bf16") > 1, mut
    # identity W: out IS bf16(y32): within the LayerNorm bound and ONE store grant; a doubled rounding is not
    eye = bf(torch.eye(d))
    y64, e_ln = R.layernorm(x, g, b)
    one = imit_lnq(x, g, b, eye, None)
    assert torch.equal(one, bf(imit_ln(x, g, b)))
    assert R.worst_ratio(one.float(), y64, e_ln, stored="bf16") <= 1
    assert R.worst_ratio(imit_lnq(x, g, b, eye, None, y_round=lambda y: bf(round7(y))).float(), y64, e_ln, stored="bf16") > 1
    for mut in LN_MUTATIONS + vec_mutations(d):
        assert R.worst_ratio(imit_lnq(x, g, b, eye, None, **mut).float(), y64, e_ln, stored="bf16") > 1, mut


# ------------------------------------------------------- stand-alone LayerNorm, exact data -------------------------------------------------------
@pytest.mark.parametrize("d", [64, 320, 768, 2048])
def test_layernorm_imitation_sits_inside_the_bound_and_the_bugs_do_not(d):
    x = R.lnq_rows(9, d, 31)
    _, g, b = R.affine(d, 32)
    for gg, bb in ((g, b), (None, None)):
        want, e = R.layernorm(x, gg, bb)
        one, zero = torch.ones(d), torch.zeros(d)
        assert R.worst_ratio(bf(imit_ln(x, gg if gg is not None else one, bb if bb is not None else zero)).float(), want, e, stored="bf16") <= 1
        assert R.worst_ratio(imit_ln(x, gg if gg is not None else one, bb if bb is not None else zero), want, e) <= 1      # the fp32 output
        for mut in LN_MUTATIONS:
            assert R.worst_ratio(bf(imit_ln(x, gg if gg is not None else one, bb if bb is not None else zero, **mut)).float(), want, e,
                                 stored="bf16") > 1, mut


@pytest.mark.parametrize("N,K", [(768, 64), (768, 768), (1024, 192)])
def test_exact_integers_are_exact_in_any_order(N, K):
    c = R.exact_operands(M, N, K, 41)
    h64, _ = R.h_ref(c["A"], c["W"], c["bias"], c["res"])
    assert torch.equal(h64.float().double(), h64)
    for rot in (0, 1, K // 32):
        assert torch.equal(imit_h(c, rot=rot).double(), h64)
    assert not torch.equal(imit_h(c, drop=0).double(), h64) and not torch.equal(imit_h(c, res_next=True).double(), h64)


def test_hashed_residual_is_the_frd_residual_tests_hash():
    r = R.hashed_residual(300, 768)
    assert torch.equal(r, bf(r).float()) and len(torch.unique(r[:128])) > 1500
    r32 = R.hashed_residual(300, 1024, bf16_exact=False)
    assert not torch.equal(r32, bf(r32).float()) and float(r32.abs().max()) < 4 and float(r32.abs().min()) >= 2.0 ** -5
