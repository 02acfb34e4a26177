"""The self-attention's residual epilogues (x = attn_out + h, reference src/components/DiT.py:131-139, no out-projection) at kernel
level, through ditto_attention_resid_bf16: every head_dim-64 residual instantiation, forced by attn_flags, on the fp32 and the bf16
stream, in place and out of place, against the fp64 reference with the elementwise bound of tests/attn_ref.py.  Padding columns
(ldr > H * dh) and rows past B * Sq hold sentinels that must come back bit for bit.  Then attn64q's exact-path redo on the
residual forms, the edges of its range contract, and the GEMM-composed path at head_dim 128.

Worst observed ratio |got - want| / bound on an MI355X (fp32 / bf16 stream; the module prints them at its end): attn64q 0.47 / 0.47,
attn64q_hold 0.39 / 0.37, attn64q_ragged 0.40 / 0.38, attn64p 0.47 / 0.47, attn64p_ring3 0.44 / 0.42, attn64v3 0.43 / 0.35,
attn64v3_8 0.30 / 0.24, attn64v2_2_4 0.35 / 0.33, attn64v2_3 0.43 / 0.35, attn64v2_2 0.35 / 0.33, attn64 (all three staging forms)
0.40 / 0.38, attn64 on pre-scaled q 0.43 / 0.36; head_dim 128 (GEMM-composed) 0.36."""
import functools
import math

import pytest
import torch

from ditto_tts_amd import hip
from attn_ref import LOG2E, bound, make_case, reference, worst_ratio
from gpu_util import asym, rel_l2, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"

# attn_flags (csrc/attention.hip:32-42): 16 pre-scaled q; 131072 never attn64p/q; 262144 attn64p/q whatever the grid; 524288 attn64p's
# ring of 3; 1048576 never attn64q; 2097152 attn64q's K-holding form on the residual epilogue; 256 never / 512 always attn64v3 (Skv %
# 128 == 0); 1024 / 2048 its 8-wave form always / never; 64 attn64v2 at 2 waves per SIMD; 128 no deep-prefetch form on small grids;
# 32 (with 16) or no 16: the older attn64_kernel, bits 0..1 its staging form.
KERNELS = {
    "attn64q": 16 + 262144,                            # attn64q_kernel<true, 0, 4, true, 0>
    "attn64q_hold": 16 + 262144 + 2097152,             # attn64q_kernel<true, 0, 4, true, 1>
    "attn64q_ragged": 16 + 262144,                     # attn64q_kernel<true, 0, 4, true, 0, true>
    "attn64p": 16 + 262144 + 1048576,                  # attn64p_kernel<true>
    "attn64p_ring3": 16 + 262144 + 524288,             # attn64p_kernel<true, 3>
    "attn64v3": 16 + 131072 + 512 + 2048,              # attn64v3_kernel<true>
    "attn64v3_8": 16 + 131072 + 512 + 1024,            # attn64v3_kernel<true, 8>
    "attn64v2_2_4": 16 + 131072 + 256,                 # attn64v2_kernel<true, 2, 4> (small grids)
    "attn64v2_3": 16 + 131072 + 256 + 128,             # attn64v2_kernel<true, 3>
    "attn64v2_2": 16 + 131072 + 256 + 64,              # attn64v2_kernel<true>
    "attn64_dma_pfv": 3,                               # attn64_kernel<true, true, true>
    "attn64_dma": 1,                                   # attn64_kernel<true, true, false>
    "attn64_regs": 0,                                  # attn64_kernel<true, false, false>
    "attn64_prescaled": 16 + 32 + 3,                   # attn64_kernel<true, true, true> on pre-scaled q
}


def route(flags, B, H, Sq, Skv):
    """Which residual instantiation launch_attention (csrc/attention.hip, attention_p.hip) picks at head_dim 64 — its rules restated."""
    if flags & 16 and not flags & 32:
        wgs = (B * Sq // 256) * H
        if not flags & 131072 and (wgs >= 768 or flags & 262144):
            if not flags & 1048576 and not flags & 524288 and Skv > 64:
                return "attn64q_ragged" if Skv % 64 else ("attn64q_hold" if flags & 2097152 else "attn64q")
            return "attn64p_ring3" if flags & 524288 else "attn64p"
        grid = -(-Sq // 128) * H * B
        if Skv % 128 == 0 and not flags & 256 and (grid <= 320 or Skv >= 2048 or flags & 512):
            return "attn64v3_8" if (flags & 1024 or (Skv >= 2048 and Sq >= 256)) and not flags & 2048 else "attn64v3"
        if not flags & 64:
            return "attn64v2_2_4" if grid <= 320 and not flags & 128 else "attn64v2_3"
        return "attn64v2_2"
    return {0: "attn64_regs", 1: "attn64_dma"}.get(flags & 3, "attn64_dma_pfv") if not flags & 16 else "attn64_prescaled"


# (B, H, Sq, Skv): Sq in {1, 63, 256, 300, 1024}, Skv in {1, 64, 65, 127, 471, 1024, 2048}; the last is a grid of 768 attn64p
# workgroups (B >= 16 at N = 1024, 12 heads: what launch_attention picks with no forcing bit)
SHAPES = [(1, 2, 1, 1), (2, 3, 63, 64), (1, 2, 256, 65), (2, 2, 300, 127), (1, 3, 300, 471), (1, 2, 1024, 1024),
          (2, 2, 63, 1024), (1, 2, 256, 2048), (16, 12, 1024, 1024)]
BIG = (16, 12, 1024, 1024)
CASES = [(name, s) for name, f in KERNELS.items() for s in SHAPES if route(f, *s) == name
         and (s != BIG or name in ("attn64q", "attn64p", "attn64v2_3", "attn64v3"))]
WORST = {}   # (kernel, stream) -> worst ratio seen in this run (printed at the end of the module)

F32_SENT, BF16_SENT = -7.0e30, 0x7FA5    # sentinels of the padding: a huge float; a NaN payload no kernel produces


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = hip.lib()
    yield lib
    hip.check(lib.ditto_set_option(b"attn_flags", 3))
    for k in sorted(WORST):
        print(f"worst ratio to the bound {k[0]:18s} {k[1]:5s} {WORST[k]:.3f}")


@functools.lru_cache(maxsize=4)
def _case(B, H, Sq, Skv):
    return make_case(B, H, Sq, Skv, seed=90 + Sq + Skv)


@functools.lru_cache(maxsize=4)
def _asym(shape, seed):
    return asym(shape, seed)


def _stream_buf(rows, cols, ldr, extra_rows, bf, data=None):
    """a [rows + extra_rows, ldr] stream buffer full of sentinels, the first `rows` x `cols` set to `data`"""
    if bf:
        t = torch.full((rows + extra_rows, ldr), BF16_SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    else:
        t = torch.full((rows + extra_rows, ldr), F32_SENT, dtype=torch.float32, device=DEV)
    if data is not None:
        t[:rows, :cols] = data.to(t.dtype)
    return t


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _run(lib, flags, q, k, v, rin, rout, ldr, bf, B, H, Sq, Skv, dh, scale, ws=None):
    d = H * dh
    try:
        hip.check(lib.ditto_set_option(b"attn_flags", flags))
        return lib.ditto_attention_resid_bf16(q.data_ptr(), d, k.data_ptr(), d, v.data_ptr(), d,
                                              None if rin is None else rin.data_ptr(), rout.data_ptr(), ldr, int(bf), B, H, Sq,
                                              Skv, dh, scale, None if ws is None else ws.data_ptr(),
                                              0 if ws is None else ws.numel(), stream())
    finally:
        torch.cuda.synchronize()
        hip.check(lib.ditto_set_option(b"attn_flags", 3))


def test_route_covers_every_residual_instantiation():
    """each instantiation of KERNELS is reached by some shape of SHAPES under its flags (so the table below is not vacuous)"""
    assert {name for name, _ in CASES} == set(KERNELS)
    assert sum(s == BIG for _, s in CASES) >= 3 and (BIG[0] * BIG[2] // 256) * BIG[1] >= 768
    assert route(16, *BIG) == "attn64q", "the model's own dispatch at the big grid"
    assert route(16, 1, 12, 1024, 1024) == "attn64v3" and route(16, 1, 12, 1024, 1000) == "attn64v2_2_4"


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-B{s[0]}H{s[1]}Sq{s[2]}Skv{s[3]}" for n, s in CASES])
def test_residual_epilogue(lib, name, shape, bf, inplace):
    B, H, Sq, Skv = shape
    flags = KERNELS[name]
    assert route(flags, B, H, Sq, Skv) == name
    dh, d = 64, H * 64
    ldr, extra = d + 8, 3
    qs, k, v, scale = _case(B, H, Sq, Skv)
    prescaled = bool(flags & 16)
    q = qs if prescaled else (qs.float() / (LOG2E * scale)).to(torch.bfloat16)   # the un-scaled kernels: q and their fp32 scale
    log2_scale = 1.0 if prescaled else scale * LOG2E
    resid = _asym((B * Sq, d), 93)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    rin = _stream_buf(B * Sq, d, ldr, extra, bf, resid.to(DEV))
    rin0 = rin.clone()
    rout = rin if inplace else _stream_buf(B * Sq, d, ldr, extra, bf)
    rout0 = rout.clone()
    assert _run(lib, flags, q, k, v, None if inplace else rin, rout, ldr, bf, B, H, Sq, Skv, dh, scale) == hip.OK, \
        hip.lib().ditto_last_error()
    o, wabs, s1 = reference(q, k, v, B, H, Sq, Skv, dh, log2_scale)
    want, e = bound(o, wabs, s1, Skv, dh, resid=rin0[:B * Sq, :d].double())
    got = rout[:B * Sq, :d]
    ratio = worst_ratio(got, want, e, bf)
    key = (name, "bf16" if bf else "fp32")
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: |got - want| exceeds the elementwise bound by {ratio:.3f}x"
    if bf:
        assert rel_l2(got, want) < 2.0 ** -8
    else:
        assert rel_l2(got - rin0[:B * Sq, :d], o) < 1.5e-2
    # padding columns and rows past B * Sq: untouched, bit for bit (and resid_in, out of place)
    assert torch.equal(_bits(rout[:, d:]), _bits(rout0[:, d:])) and torch.equal(_bits(rout[B * Sq:]), _bits(rout0[B * Sq:]))
    if not inplace:
        assert torch.equal(_bits(rin), _bits(rin0)), "resid_in written"


def _range_case(case, B, H, Sq, Skv):
    """test_gpu_kernels.py's out-of-range inputs (pre-scaled q, log2 units), generalised to Sq = 300: the workgroups that must fall back"""
    dh = 64
    q = asym((B * Sq, H * dh), 61) * 0.7
    k = asym((B * Skv, H * dh), 62) * 0.7
    v = asym((B * Skv, H * dh), 63)
    qs = q * (LOG2E / 8.0)
    u = torch.full((dh,), 0.125)
    nwg = -(-Sq // 256)
    fb = torch.zeros(B, H, nwg, dtype=torch.bool)
    if case == "overflow":
        qs = qs * 60.0
        fb[:] = True
    elif case == "underflow":
        k[:, :] = u.repeat(H) + 0.02 * k
        qs = -150.0 * u.repeat(H) + 0.3 * qs
        fb[:] = True
    elif case == "nan":
        qs[260, dh:2 * dh] = float("nan")      # batch 0, head 1, workgroup 1
        fb[0, 1, 1] = True
    else:
        qs[Sq + 256:2 * Sq, 2 * dh:3 * dh] *= 60.0      # batch 1, head 2, workgroup 1 overflows
        qs[10, :dh] = -150.0 * u                        # batch 0, head 0, one row underflows against keys ~ u
        k[:Skv, :dh] = u + 0.02 * k[:Skv, :dh]
        fb[1, 2, 1] = True
        fb[0, 0, 0] = True
    return qs.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), fb


def _per_wg(x, B, H, Sq, dh=64):
    """[B*Sq, H*dh] -> [B, H, Sq, dh] (the workgroup of row i is i // 256)"""
    return x.reshape(B, Sq, H, dh).permute(0, 2, 1, 3)


def _wg_mask(fb, Sq):
    return fb.repeat_interleave(256, dim=2)[:, :, :Sq]      # [B, H, Sq]


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Sq", [512, 300])
@pytest.mark.parametrize("Skv", [512, 471])
@pytest.mark.parametrize("case", ["overflow", "underflow", "nan", "mixed"])
def test_residual_redo_on_the_exact_path(lib, case, Skv, Sq, bf, inplace):
    """attn64q's residual forms (the bf16 one stages its stream rows by LDS-DMA into two dead ring slots and hands that LDS to
    attn64p_body on a redo): a workgroup whose rows left the range is attn64p's result bit for bit — the residual added once —
    and every other workgroup stays within the bound."""
    B, H, dh = 2, 4, 64
    d, ldr = H * dh, H * dh + 8
    qs, k, v, fb = _range_case(case, B, H, Sq, Skv)
    qs, k, v = qs.to(DEV), k.to(DEV), v.to(DEV)
    resid = asym((B * Sq, d), 95).to(DEV)
    outs = []
    for flags in (16 + 262144, 16 + 262144 + 1048576):      # attn64q (Skv > 64: this shape), attn64p
        assert route(flags, B, H, Sq, Skv) in (("attn64q_ragged" if Skv % 64 else "attn64q"), "attn64p")
        rin = _stream_buf(B * Sq, d, ldr, 2, bf, resid)
        rout = rin if inplace else _stream_buf(B * Sq, d, ldr, 2, bf)
        rout0 = rout.clone()
        assert _run(lib, flags, qs, k, v, None if inplace else rin, rout, ldr, bf, B, H, Sq, Skv, dh, 1.0 / 8) == hip.OK
        assert torch.equal(_bits(rout[:, d:]), _bits(rout0[:, d:])) and torch.equal(_bits(rout[B * Sq:]), _bits(rout0[B * Sq:]))
        outs.append(rout[:B * Sq, :d])
    got, exact = (_per_wg(x, B, H, Sq) for x in outs)
    m = _wg_mask(fb, Sq).to(DEV)
    r0 = _stream_buf(B * Sq, d, ldr, 0, bf, resid)[:, :d]
    assert torch.equal(_bits(got.contiguous())[m], _bits(exact.contiguous())[m]), "a workgroup out of range is not the exact path's"
    o, wabs, s1 = reference(qs, k, v, B, H, Sq, Skv, dh)
    want, e = bound(o, wabs, s1, Skv, dh, resid=r0.double())
    want, e = _per_wg(want, B, H, Sq), _per_wg(e, B, H, Sq)
    ok = ~m
    if case != "nan":
        assert worst_ratio(exact, want, e, bf) <= 1.0, "attn64p outside the bound"
    assert worst_ratio(got[ok], want[ok], e[ok], bf) <= 1.0
    if case in ("nan", "mixed") and not bf:     # (on the bf16 stream the two paths' fp32 differences mostly round away)
        assert not torch.equal(got[ok], exact[ok]), "expected the optimistic path on the workgroups inside the range"


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Skv", [512, 471])
def test_range_contract_boundary(lib, Skv, bf):
    """The range contract: attn64q's optimistic path holds while every row sum of exp2(s) lies in [2^-100, 2^100] (s = q.k * scale *
    log2(e)).  One row per workgroup with log2 l = -98, +98 (inside: the optimistic path, within the bound at its edge) and -102,
    +102 (outside: the workgroup redoes on the exact path and is attn64p's bit for bit)."""
    B, H, Sq, dh = 1, 1, 1024, 64
    targets = {100: -98.0, 356: 98.0, 612: -102.0, 868: 102.0}     # row -> log2 of its row sum
    k = (torch.full((Skv, dh), 0.125) + 0.004 * asym((Skv, dh), 97)).to(torch.bfloat16)
    v = asym((Skv, dh), 98).to(torch.bfloat16)
    qf = asym((Sq, dh), 96) * (0.7 * LOG2E / 8.0)
    u = torch.full((dh,), 0.125, dtype=torch.float64)
    for row, L in targets.items():
        c = L - math.log2(Skv)
        for _ in range(4):            # the bf16 rounding of q moves the sum: solve for the scale on the rounded row
            qr = (c * u).to(torch.bfloat16)
            s = qr.double() @ k.double().T
            lg = float(torch.logsumexp(s * math.log(2.0), 0)) / math.log(2.0)
            c += L - lg
        qf[row] = qr.float()
        assert abs(lg - L) < 0.5, (row, lg)
    qs = qf.to(torch.bfloat16).to(DEV)
    k, v = k.to(DEV), v.to(DEV)
    resid = asym((Sq, dh), 99).to(DEV)
    outs = []
    for flags in (16 + 262144, 16 + 262144 + 1048576):
        rin = _stream_buf(Sq, dh, dh + 8, 1, bf, resid)
        assert _run(lib, flags, qs, k, v, None, rin, dh + 8, bf, B, H, Sq, Skv, dh, 1.0 / 8) == hip.OK
        outs.append(rin[:Sq, :dh])
    got, exact = outs
    o, wabs, s1 = reference(qs, k, v, B, H, Sq, Skv, dh)
    want, e = bound(o, wabs, s1, Skv, dh, resid=_stream_buf(Sq, dh, dh, 0, bf, resid).double())
    assert worst_ratio(exact, want, e, bf) <= 1.0
    for row, L in targets.items():
        wg = slice(row // 256 * 256, row // 256 * 256 + 256)
        if abs(L) < 100:
            assert worst_ratio(got[wg], want[wg], e[wg], bf) <= 1.0, f"log2 l = {L}: optimistic path outside the bound"
            if not bf:
                assert not torch.equal(got[wg], exact[wg]), f"log2 l = {L}: expected the optimistic path"
        else:
            assert torch.equal(_bits(got[wg].contiguous()), _bits(exact[wg].contiguous())), f"log2 l = {L}: expected the exact path"


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("B,H,Sq,Skv", [(1, 2, 300, 471), (2, 1, 63, 128)])
def test_residual_at_head_dim_128(lib, B, H, Sq, Skv, inplace):
    """head_dim 128: the GEMM-composed path with its fp32 residual epilogue (scores in fp32, bf16 probabilities normalised before P V);
    a bf16 stream there is refused and the stream left untouched."""
    dh = 128
    d, ldr = H * dh, H * dh + 8
    scale = 1.0 / math.sqrt(dh)
    q = (asym((B * Sq, d), 101) * 2.0).to(torch.bfloat16).to(DEV)
    k = asym((B * Skv, d), 102).to(torch.bfloat16).to(DEV)
    v = asym((B * Skv, d), 103).to(torch.bfloat16).to(DEV)
    resid = asym((B * Sq, d), 104).to(DEV)
    ws = torch.empty(max(lib.ditto_attention_workspace_bytes(B, H, Sq, Skv, dh), 16), dtype=torch.uint8, device=DEV)
    rin = _stream_buf(B * Sq, d, ldr, 2, False, resid)
    rin0 = rin.clone()
    rout = rin if inplace else _stream_buf(B * Sq, d, ldr, 2, False)
    rout0 = rout.clone()
    assert _run(lib, 3, q, k, v, None if inplace else rin, rout, ldr, False, B, H, Sq, Skv, dh, scale, ws) == hip.OK
    o, wabs, s1 = reference(q, k, v, B, H, Sq, Skv, dh, scale * LOG2E)
    want, e = bound(o, wabs, s1, Skv, dh, resid=rin0[:B * Sq, :d].double())
    ratio = worst_ratio(rout[:B * Sq, :d], want, e)
    WORST[("generic_dh128", "fp32")] = max(WORST.get(("generic_dh128", "fp32"), 0.0), ratio)
    assert ratio <= 1.0
    assert torch.equal(_bits(rout[:, d:]), _bits(rout0[:, d:])) and torch.equal(_bits(rout[B * Sq:]), _bits(rout0[B * Sq:]))
    if not inplace:
        assert torch.equal(_bits(rin), _bits(rin0))
    # the bf16 stream exists on the fused head_dim-64 kernels only
    rb = _stream_buf(B * Sq, d, ldr, 2, True, resid)
    rb0 = rb.clone()
    assert _run(lib, 3, q, k, v, None, rb, ldr, True, B, H, Sq, Skv, dh, scale, ws) != hip.OK
    assert torch.equal(_bits(rb), _bits(rb0)), "a refused call wrote the stream"
