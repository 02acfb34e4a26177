"""Packed attention at kernel level (ditto_attention_packed_bf16 / ditto_attention_resid_packed_bf16): utterances concatenated along
the rows, utterance b in query rows [cu_q[b], cu_q[b+1]) and key rows [cu_kv[b], cu_kv[b+1]), on both routes (attn64q with attn64p's
body for one-tile utterances; attn_flags 1048576: attn64p alone), the plain form and the residual form on the fp32 and the bf16
stream.  Every row is checked against fp64 on its utterance's rows with the elementwise bound of tests/attn_ref.py and must be bit for
bit what the padded varlen kernel gives the same utterance.  The packed buffers sit between NaN / sentinel rows: those rows must
stay untouched and must not reach any result."""
import pytest
import torch

from ditto_tts_amd import hip, varlen
from attn_ref import bound, make_case, reference, worst_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, NP = 2, 1000                   # padded length of the varlen reference batch
QLEN = [1, 63, 64, 65, 1000, 300, 129, 200]
KVLEN = [65, 1000, 1, 64, 63, 300, 200, 129]     # (offsets are not multiples of 64: most utterances start mid-tile)
B = len(QLEN)
ROUTES = {"attn64q": 16 + 262144, "attn64p": 16 + 262144 + 1048576}
FORMS = ["plain", "resid_f32", "resid_bf16"]
F32_SENT, BF16_SENT = -7.0e30, 0x7FA5
GUARD = 70                         # sentinel rows on either side of every packed buffer


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = hip.lib()
    yield lib
    hip.check(lib.ditto_set_option(b"attn_flags", 3))


def _padded(seed):
    q, k, v, _ = make_case(B, H, NP, NP, seed=seed)
    return q.view(B, NP, H * 64), k.view(B, NP, H * 64), v.view(B, NP, H * 64)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _guarded(packed, fill):
    """packed [S, C] placed between GUARD rows of `fill` on either side (a bf16 fill is a raw bit pattern); returns (buffer, view)"""
    S, Cn = packed.shape
    if packed.dtype == torch.bfloat16 and isinstance(fill, int):
        buf = torch.full((S + 2 * GUARD, Cn), fill, dtype=torch.int16).view(torch.bfloat16)
    else:
        buf = torch.full((S + 2 * GUARD, Cn), fill, dtype=packed.dtype)
    buf[GUARD:GUARD + S] = packed
    buf = buf.to(DEV)
    return buf, buf[GUARD:GUARD + S]


def _resid(form, seed=3):
    r = torch.randn(B, NP, H * 64, generator=torch.Generator().manual_seed(seed))
    return r.to(torch.bfloat16) if form == "resid_bf16" else r


def _run_packed(lib, route, form, q, k, v, rin=None):
    """padded inputs -> (packed result [S, H*64] CPU, the whole guarded output buffer CPU); q / k / v / resid_in sit between NaN rows"""
    qp, cq = varlen.pack(q, QLEN)
    kp, ck = varlen.pack(k, KVLEN)
    vp, _ = varlen.pack(v, KVLEN)
    nan = float("nan")
    _, qv = _guarded(qp, nan)
    _, kv = _guarded(kp, nan)
    _, vv = _guarded(vp, nan)
    hip.check(lib.ditto_set_option(b"attn_flags", ROUTES[route]))
    try:
        if form == "plain":
            obuf, ov = _guarded(torch.zeros(qp.shape[0], H * 64, dtype=torch.bfloat16), BF16_SENT)
            varlen.attention_packed(qv, kv, vv, H, cq, ck, max(QLEN), max(KVLEN), out=ov)
        else:
            rp, _ = varlen.pack(rin, QLEN)
            _, rv = _guarded(rp, nan)
            sent = F32_SENT if form == "resid_f32" else BF16_SENT
            obuf, ov = _guarded(torch.zeros_like(rp), sent)
            varlen.attention_resid_packed(qv, kv, vv, H, ov, cq, ck, max(QLEN), max(KVLEN), resid_in=rv)
        torch.cuda.synchronize()
        return ov.cpu(), obuf.cpu(), cq.cpu()
    finally:
        hip.check(lib.ditto_set_option(b"attn_flags", 3))


def _run_varlen(lib, route, form, q, k, v, rin=None):
    hip.check(lib.ditto_set_option(b"attn_flags", ROUTES[route]))
    try:
        if form == "plain":
            out = torch.zeros(B, NP, H * 64, dtype=torch.bfloat16, device=DEV)
            varlen.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, QLEN, KVLEN, out=out)
        else:
            out = torch.zeros_like(rin).to(DEV)
            varlen.attention_resid(q.to(DEV), k.to(DEV), v.to(DEV), H, out, QLEN, KVLEN, resid_in=rin.to(DEV))
        torch.cuda.synchronize()
        return out.cpu()
    finally:
        hip.check(lib.ditto_set_option(b"attn_flags", 3))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_packed_against_fp64_and_varlen_bits(lib, route, form):
    q, k, v = _padded(7)
    rin = None if form == "plain" else _resid(form)
    got, buf, cq = _run_packed(lib, route, form, q, k, v, rin)
    pad = _run_varlen(lib, route, form, q, k, v, rin)
    worst = 0.0
    for b, (n, m) in enumerate(zip(QLEN, KVLEN)):
        g = got[int(cq[b]):int(cq[b + 1])]
        o, wabs, s1 = reference(q[b, :n], k[b, :m], v[b, :m], 1, H, n, m, 64)
        want, e = bound(o, wabs, s1, m, 64, None if rin is None else rin[b, :n])
        r = worst_ratio(g, want, e, stored_bf16=form != "resid_f32")
        assert r <= 1.0, f"utterance {b} (q {n}, kv {m}): worst |got - want| / bound {r:.3f}"
        worst = max(worst, r)
        assert torch.equal(_bits(g), _bits(pad[b, :n])), f"utterance {b}: not the padded varlen kernel's bits"
    # the guard rows around the output are untouched
    guard = torch.cat([buf[:GUARD], buf[-GUARD:]])
    if form == "resid_f32":
        assert (guard == F32_SENT).all(), "a guard row around the packed stream was written"
    else:
        assert (_bits(guard) == BF16_SENT).all(), "a guard row around the packed output was written"
    print(f"{route} {form}: worst ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("route", list(ROUTES))
def test_guard_rows_and_neighbours_reach_nothing(lib, route):
    """the same utterances with other data in every OTHER utterance and NaN guards: each utterance's bits are unchanged"""
    q, k, v = _padded(11)
    a, _, cq = _run_packed(lib, route, "plain", q, k, v)
    q2, k2, v2 = _padded(12)
    q2[3], k2[3], v2[3] = q[3], k[3], v[3]
    b_, _, _ = _run_packed(lib, route, "plain", q2, k2, v2)
    s = slice(int(cq[3]), int(cq[4]))
    assert torch.equal(_bits(a[s]), _bits(b_[s]))
    assert torch.isfinite(a.float()).all() and torch.isfinite(b_.float()).all()


def test_offsets_are_validated_before_the_launch(lib):
    q, k, v = _padded(7)
    qp, cq = varlen.pack(q, QLEN)
    kp, ck = varlen.pack(k, KVLEN)
    qp, kp = qp.to(DEV), kp.to(DEV)
    bad_start = cq.clone(); bad_start[0] = 1
    with pytest.raises(ValueError):
        varlen.attention_packed(qp, kp, kp, H, bad_start, ck)
    with pytest.raises(ValueError):
        varlen.attention_packed(qp, kp, kp, H, cq, ck, max_kv=999)
    with pytest.raises(ValueError):
        varlen.attention_packed(qp, kp, kp, H, cq.float(), ck)
