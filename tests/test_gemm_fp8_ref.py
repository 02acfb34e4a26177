"""Keeps tests/gemm_fp8_ref.py honest without a GPU.  An fp32 emulation of the fp8 GEMM's arithmetic (fp32 partial sums per 128-deep
step added in fp32, scale, then bias, the fp32 epilogue, ONE round-to-nearest-even store through torch's cast) on the data families
test_gpu_gemm_fp8.py uses, at their smallest shapes: worst_ratio <= 1, so each bound admits a right implementation before it meets
the kernel; and the same emulation with each modelled bug: worst_ratio > 1, so each bound refuses a wrong one.  -s prints the ratios."""
import math

import pytest
import torch

import gemm_epi_ref as E
import gemm_fp8_ref as R


def _f32(u8):
    return u8.view(torch.float8_e4m3fn).float()


def acc32(Aq, Wq, bug=None):
    A, W = _f32(Aq), _f32(Wq)
    steps = [A[:, k:k + 128] @ W[:, k:k + 128].T for k in range(0, A.shape[1], 128)]
    if bug == "last_ktile_dropped":
        steps = steps[:-1] or [torch.zeros_like(steps[0])]
    if bug == "last_ktile_twice":
        steps = steps + steps[-1:]
    acc = steps[0]
    for s in steps[1:]:
        acc = acc + s
    return acc


def pre32(Aq, Wq, ws, b, bug=None):
    """the fp32 value the epilogue starts from"""
    acc = acc32(Aq, Wq, bug)
    N = ws.shape[0]
    n = torch.arange(N)
    if bug == "scales_of_neighbour_tile":                      # tile t ^ 1 where it exists, same in-tile offset
        m = (n // 256 ^ 1) * 256 + n % 256
        ws = ws[torch.where(m < N, m, n)]
    if bug == "scales_shifted_4":
        ws = ws[(n + 4) % N]
    if bug == "scale_after_bias":
        return (acc + b) * ws
    return acc * ws + b


def trunc_e4m3(y):
    """saturating conversion that rounds toward zero: one code below the RNE result wherever that one lies beyond y"""
    q = R.to_e4m3(y)
    over = R.deq(q).abs() > y.double().clamp(-448, 448).abs()
    return torch.where(over, q - 1, q)                          # sign-magnitude codes: - 1 is one step toward zero


def gated32(pre, bug=None):
    a, g = E.deinterleave(pre)
    if bug == "fc1_gate_exchanged":
        a, g = g, a
    y = torch.nn.functional.gelu(a) * torch.sigmoid(g)
    if bug == "truncation":
        q = trunc_e4m3(y)
    elif bug == "non_saturating":
        q = y.to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        q = R.to_e4m3(y)
    if bug == "store_halves_exchanged":
        q = q.reshape(q.shape[0], -1, 2, 4).flip(2).reshape(q.shape)
    return q


def rope32(pre, M, rpb, rc, bug=None):
    """table-free angles as the kernel forms them, a correctly rounded v_sin / v_cos, the rotation in fp32"""
    invf = E.inv_freq()
    pos = torch.arange(M) if bug == "position_is_row" else torch.arange(M) % rpb
    t = pos.float()[:, None] * E.freq_rev(invf)[None, :]
    rev = (t - t.floor()).double() * 2 * math.pi
    c, s = rev.cos().float()[:, None, :], rev.sin().float()[:, None, :]
    if bug == "sine_sign":
        s = -s
    if bug == "pair_16":                                        # (j, j + 16): blocks (0, 1) and (2, 3) of a head instead of (0, 2), (1, 3)
        h = pre[:, :rc].reshape(M, rc // 64, 2, 2, 16)
        lo, hi = h[:, :, :, 0].reshape(M, rc // 64, 32), h[:, :, :, 1].reshape(M, rc // 64, 32)
        o = torch.stack([(lo * c - hi * s).reshape(M, -1, 2, 16), (hi * c + lo * s).reshape(M, -1, 2, 16)], dim=3)
        return torch.cat([o.reshape(M, rc), pre[:, rc:]], dim=1)
    lo, hi = E._split(pre, rc)
    return E._join(lo * c - hi * s, hi * c + lo * s, pre[:, rc:])


PLAIN_BUGS = ["scales_of_neighbour_tile", "scales_shifted_4", "scale_after_bias", "last_ktile_dropped", "last_ktile_twice"]
GATED_BUGS = ["fc1_gate_exchanged", "store_halves_exchanged", "truncation", "non_saturating"]
ROPE_BUGS = ["sine_sign", "pair_16", "position_is_row"]


def test_e4m3_grant_is_half_an_ulp_of_torchs_cast():
    g = torch.Generator().manual_seed(1)
    y = torch.exp(torch.rand(10 ** 6, generator=g, dtype=torch.float64) * (math.log(448) - math.log(1e-3)) + math.log(1e-3)).float()
    y = torch.cat([y, -y[:1000], torch.zeros(1)])
    codes = R.deq(torch.arange(0x7F, dtype=torch.uint8)).float()                 # every non-negative finite e4m3 value, ascending
    ties = (codes[:-1] + codes[1:]) / 2
    for v, exact_one in ((y, False), (ties, True)):
        got = R.deq(R.to_e4m3(v))
        r = ((got - v.double()).abs() / R.half_ulp_e4m3(got)).max()
        assert float(r) <= 1.0
        if exact_one:
            assert float(r) == 1.0
    # saturation and NaN bytes
    zero = torch.full((3,), 1e-30, dtype=torch.float64)
    assert R.worst_ratio(R.deq(R.to_e4m3(torch.tensor([500.0, -1e9, 448.0]))), torch.tensor([500.0, -1e9, 448.0], dtype=torch.float64),
                         zero, stored="e4m3") == 0.0
    assert R.worst_ratio(R.deq(torch.tensor([0x7F], dtype=torch.uint8)), torch.ones(1, dtype=torch.float64), zero[:1], stored="e4m3") == math.inf
    assert R.worst_ratio(R.deq(torch.tensor([0xFF], dtype=torch.uint8)), torch.ones(1, dtype=torch.float64), zero[:1], stored="e4m3") == math.inf
    assert float(R.half_ulp_e4m3(torch.tensor([0.0, 2.0 ** -9, 2.0 ** -6, 1.0, 448.0], dtype=torch.float64)).sub(
        torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -4, 16.0], dtype=torch.float64)).abs().max()) == 0.0


def test_scales_differ_by_decades_between_neighbours():
    """what makes a scale from the wrong column or the wrong tile visible: the data, not the bound"""
    _, _, ws, b = R.operands(8, 2336, 128, 31)
    for shift in (4, 256):
        ratio = (ws[shift:] / ws[:-shift]).log10().abs()
        assert float(ratio.median()) > 0.5 and float((ratio > 1).float().mean()) > 0.25, (shift, float(ratio.median()))


@pytest.mark.parametrize("M,N,K", [(64, 16, 128), (300, 320, 128), (513, 2336, 384)])
def test_fp32_plain_epilogues_sit_inside_the_bound_and_the_bugs_do_not(M, N, K):
    Aq, Wq, ws, b = R.operands(M, N, K, 31)
    want, accb = R.linear(Aq, Wq, ws, b)
    ldr, ldo = N + 12, N + 24
    g = torch.Generator().manual_seed(2)
    resbuf = torch.randn(2 * M, ldr, generator=g)               # (rows to spare for the wrong stride)
    rows, cols = torch.arange(M)[:, None], torch.arange(N)[None, :]

    def ratios(bug=None):
        v = pre32(Aq, Wq, ws, b, bug)
        res = resbuf.flatten()[rows * (ldo if bug == "residual_at_ldo" else ldr) + cols]
        wres = want + resbuf[:M, :N].double()
        return {"f32": R.worst_ratio(v, want, accb), "bf16": R.worst_ratio(v.to(torch.bfloat16), want, accb, stored="bf16"),
                "res": R.worst_ratio(v + res, wres, accb + 2 * R.G * wres.abs())}
    ok = ratios()
    print(f"plain M {M} N {N} K {K}: " + "  ".join(f"{k} {v:.3f}" for k, v in ok.items()))
    assert max(ok.values()) <= 1.0, ok
    assert ratios("residual_at_ldo")["res"] > 1.0
    for bug in PLAIN_BUGS:
        if (bug == "scales_of_neighbour_tile" and N <= 256) or (bug == "scales_shifted_4" and N <= 16):
            continue                                            # one tile / one 16-column block: the bug has nothing to confuse
        if bug == "last_ktile_dropped" and K // 128 % 2 == 0:
            continue
        r = ratios(bug)
        print(f"   {bug}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert min(r.values()) > 1.0, (bug, r)
    if K == 384:
        assert K // 128 % 2 == 1                                # the dropped K-tile was tried at an odd K-tile count


@pytest.mark.parametrize("M,N,K", [(300, 320, 128), (513, 2336, 384)])
def test_fp32_gated_epilogue_sits_inside_the_bound_and_the_bugs_do_not(M, N, K):
    Aq, Wq, ws, b = R.operands(M, N, K, 41, gated_data=True)
    pre, accb = R.linear(Aq, Wq, ws, b)
    want, bound = R.gated(pre), R.gated_bound(pre, accb)
    sat, sub = R.e4m3_edges(want)
    assert sat >= 32 and sub >= 32, (sat, sub)
    ok = R.worst_ratio(R.deq(gated32(pre32(Aq, Wq, ws, b))), want, bound, stored="e4m3")
    print(f"gated M {M} N {N} K {K}: {ok:.3f} ({sat} saturate, {sub} subnormal)")
    assert ok <= 1.0
    for bug in GATED_BUGS:
        r = R.worst_ratio(R.deq(gated32(pre32(Aq, Wq, ws, b), bug)), want, bound, stored="e4m3")
        print(f"   {bug}: {r:.3g}")
        assert r > 1.0, bug
    for bug in PLAIN_BUGS:
        if bug == "last_ktile_dropped" and K // 128 % 2 == 0:
            continue
        r = R.worst_ratio(R.deq(gated32(pre32(Aq, Wq, ws, b, bug))), want, bound, stored="e4m3")
        print(f"   {bug}: {r:.3g}")
        assert r > 1.0, bug


@pytest.mark.parametrize("d,rpb,M", [(256, 64, 63), (256, 200, 600)])
def test_fp32_rope_epilogue_sits_inside_the_bound_and_the_bugs_do_not(d, rpb, M):
    N, K, rc = 3 * d, d, 2 * d
    Aq, Wq, ws, b = R.operands(M, N, K, 51)
    pre, accb = R.linear(Aq, Wq, ws, b)
    invf = E.inv_freq()
    pos = torch.arange(M) % rpb
    c64, s64 = E.rope_exact_tables(invf, pos)
    want = R.rope(pre, torch.arange(M), rc, c64, s64)
    bound = R.rope_bound(pre, accb, rc, R.dtheta_table_free(pos, invf), E.E_SINCOS)
    p32 = pre32(Aq, Wq, ws, b)
    ok = R.worst_ratio(rope32(p32, M, rpb, rc).to(torch.bfloat16), want, bound, stored="bf16")
    # from tables: the reference reads the same fp32 tables
    cs, sn = E.tables(invf, rpb)
    lo, hi = E._split(p32, rc)
    tab = E._join(lo * cs[pos][:, None] - hi * sn[pos][:, None], hi * cs[pos][:, None] + lo * sn[pos][:, None], p32[:, rc:])
    ok_tab = R.worst_ratio(tab.to(torch.bfloat16), R.rope(pre, pos, rc, cs, sn), R.rope_bound(pre, accb, rc), stored="bf16")
    print(f"rope d {d} rpb {rpb} M {M}: table-free {ok:.3f} tables {ok_tab:.3f}")
    assert ok <= 1.0 and ok_tab <= 1.0
    for bug in ROPE_BUGS:
        if bug == "position_is_row" and M <= rpb:
            continue                                            # one utterance: row IS the position
        r = R.worst_ratio(rope32(p32, M, rpb, rc, bug).to(torch.bfloat16), want, bound, stored="bf16")
        print(f"   {bug}: {r:.3g}")
        assert r > 1.0, bug
    for bug in PLAIN_BUGS[:3]:
        r = R.worst_ratio(rope32(pre32(Aq, Wq, ws, b, bug), M, rpb, rc).to(torch.bfloat16), want, bound, stored="bf16")
        assert r > 1.0, bug


def test_exact_integer_data_need_no_bound():
    """every partial sum is exactly representable: the fp32 emulation IS the fp64 reference, in any order"""
    M, N, K = 300, 320, 384
    Aq, Wq, ws, b = R.exact_operands(M, N, K, 61)
    want, _ = R.linear(Aq, Wq, ws, b)
    got = pre32(Aq, Wq, ws, b)
    assert torch.equal(got.double(), want) and torch.equal(want.float().double(), want)
    assert float(want.abs().max()) > 100 and len(set(ws.tolist())) == 7
    for bug in PLAIN_BUGS:
        assert not torch.equal(pre32(Aq, Wq, ws, b, bug).double(), want), bug


@pytest.mark.parametrize("d", [64, 320, 2048])
@pytest.mark.parametrize("affine", [True, False])
def test_fp32_layernorm_sits_inside_the_bound(d, affine):
    x, g, b = R.layernorm_data(5, d, 71)
    if not affine:
        g = b = None
    want, e = R.layernorm(x, g, b)
    got = torch.nn.functional.layer_norm(x, (d,), g, b, 1e-5)
    r = R.worst_ratio(R.deq(R.to_e4m3(got)), want, e, stored="e4m3")
    print(f"layernorm d {d} affine {affine}: {r:.3f}")
    assert r <= 1.0
    if affine:
        assert int((want.abs() > 448).sum()) >= 4                 # the scaled gamma columns saturate
    assert float(x[-1].min()) == float(x[-1].max())               # the constant row
    # a variance that forgets the mean (E[x^2] instead of E[(x - mean)^2]) is refused
    bad = x / torch.sqrt((x * x).mean(dim=1, keepdim=True) + 1e-5) * (g if affine else 1.0) + (b if affine else 0.0)
    assert R.worst_ratio(R.deq(R.to_e4m3(bad)), want, e, stored="e4m3") > 1.0


@pytest.mark.parametrize("rows,cols", [(1, 4), (5, 132), (200, 384), (7, 1028)])
def test_torch_quantiser_sits_inside_the_bound(rows, cols):
    x = R.quantize_data(rows, cols, 81)
    q, sc = R.quantize_rows(x)
    err, bound = R.quantize_bound(x, q, sc)
    assert bool((err <= bound).all())
    # a truncating quantiser is refused
    errt, _ = R.quantize_bound(x, trunc_e4m3(x * (1.0 / sc)[:, None]), sc)
    if rows * cols > 64:
        assert not bool((errt <= bound).all())
