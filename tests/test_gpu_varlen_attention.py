"""Variable-length attention at kernel level (ditto_attention_varlen_bf16 / ditto_attention_resid_varlen_bf16): per-utterance query and
key lengths in the padded layout, on both routes (attn64q with attn64p's body for one-tile utterances; attn_flags 1048576: attn64p
alone), the plain form and the residual form on the fp32 and the bf16 stream.  Every valid row is checked against fp64 on that
utterance's own rows with the elementwise bound of tests/attn_ref.py; rows past q_len must come back bit for bit; NaN in any padding
(q, k, v, stream) must change no valid bit; an utterance's bits must not depend on its neighbours, its position or the padded length."""
import pytest
import torch

from ditto_tts_amd import hip, varlen
from attn_ref import bound, make_case, reference, worst_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, SQ, SKV = 2, 600, 600          # padded lengths: 600 % 256 != 0 (a partial last query block of the padded grid as well)
QLEN = [1, 63, 64, 65, 127, 128, 300, 471, 600]
KVLEN = [471, 65, 1, 600, 64, 300, 127, 63, 128]
B = len(QLEN)
ROUTES = {"attn64q": 16 + 262144, "attn64p": 16 + 262144 + 1048576}
FORMS = ["plain", "resid_f32", "resid_bf16"]
F32_SENT, BF16_SENT = -7.0e30, 0x7FA5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = hip.lib()
    assert hip.has_varlen()
    yield lib
    hip.check(lib.ditto_set_option(b"attn_flags", 3))


def _case(seed=7, Sq=SQ, Skv=SKV, Bn=B):
    q, k, v, _ = make_case(Bn, H, Sq, Skv, seed=seed)
    return q.view(Bn, Sq, H * 64), k.view(Bn, Skv, H * 64), v.view(Bn, Skv, H * 64)


def _resid(form, Bn=B, Sq=SQ, seed=3):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(Bn, Sq, H * 64, generator=g)
    return r.to(torch.bfloat16) if form == "resid_bf16" else r


def _sentinel(form, Bn=B, Sq=SQ):
    if form == "resid_f32":
        return torch.full((Bn, Sq, H * 64), F32_SENT, dtype=torch.float32)
    return torch.full((Bn, Sq, H * 64), BF16_SENT, dtype=torch.int16).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _run(lib, route, form, q, k, v, ql, kl, resid_in=None, out_init=None):
    """one launch; returns the output / stream buffer (CPU).  Rows past q_len of the buffer start as `out_init` (default sentinels)."""
    hip.check(lib.ditto_set_option(b"attn_flags", ROUTES[route]))
    try:
        Bn, Sq = q.shape[0], q.shape[1]
        q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
        if form == "plain":
            out = (_sentinel(form, Bn, Sq) if out_init is None else out_init).to(DEV)
            varlen.attention(q, k, v, H, ql, kl, out=out)
        else:
            # out of place: the stream buffer starts as sentinels past q_len (they must survive), resid_in holds the stream
            out = (_sentinel(form, Bn, Sq) if out_init is None else out_init).to(DEV)
            varlen.attention_resid(q, k, v, H, out, ql, kl, resid_in=resid_in.to(DEV))
        torch.cuda.synchronize()
        return out.cpu()
    finally:
        hip.check(lib.ditto_set_option(b"attn_flags", 3))


def _with_nan_padding(x, lens):
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, n:] = float("nan")
    return x


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_varlen_against_fp64_per_utterance(lib, route, form):
    q, k, v = _case()
    rin = None if form == "plain" else _resid(form)
    got = _run(lib, route, form, q, k, v, QLEN, KVLEN, resid_in=rin)
    sent = _sentinel(form)
    worst = 0.0
    for b, (n, m) in enumerate(zip(QLEN, KVLEN)):
        o, wabs, s1 = reference(q[b, :n], k[b, :m], v[b, :m], 1, H, n, m, 64)
        want, e = bound(o, wabs, s1, m, 64, None if rin is None else rin[b, :n])
        r = worst_ratio(got[b, :n], want, e, stored_bf16=form != "resid_f32")
        assert r <= 1.0, f"utterance {b} (q_len {n}, kv_len {m}): worst |got - want| / bound {r:.3f}"
        worst = max(worst, r)
        assert torch.equal(_bits(got[b, n:]), _bits(sent[b, n:])), f"utterance {b}: a row past q_len = {n} was written"
    print(f"{route} {form}: worst ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_nan_padding_reaches_no_valid_row(lib, route, form):
    """NaN in every padding row of q, k, v and the stream: the valid rows are bit for bit those of the zero-padded run (0 * NaN =
    NaN in P V: a padded K / V row that was read would show)"""
    q, k, v = _case(seed=11)
    zq, zk, zv = (_with_nan_padding(x, L).nan_to_num(0.0) for x, L in ((q, QLEN), (k, KVLEN), (v, KVLEN)))
    nq, nk, nv = _with_nan_padding(q, QLEN), _with_nan_padding(k, KVLEN), _with_nan_padding(v, KVLEN)
    rin = None if form == "plain" else _resid(form)
    a = _run(lib, route, form, zq, zk, zv, QLEN, KVLEN, resid_in=rin)
    b_ = _run(lib, route, form, nq, nk, nv, QLEN, KVLEN, resid_in=None if rin is None else _with_nan_padding(rin, QLEN))
    for b, n in enumerate(QLEN):
        assert torch.equal(_bits(a[b, :n]), _bits(b_[b, :n])), f"utterance {b}: padding changed a valid row"
        assert torch.isfinite(b_[b, :n].float()).all()


@pytest.mark.parametrize("route", list(ROUTES))
def test_nan_in_padded_query_rows_changes_nothing(lib, route):
    """NaN only in the padded query rows: nothing changes.  This covers the clamped query load (a padded row reads row q_len - 1,
    never its own data); it cannot see the range check's qvalid gate, which only matters if a padded row's data were loaded."""
    q, k, v = _case(seed=13)
    a = _run(lib, route, "plain", q, k, v, QLEN, KVLEN)
    b_ = _run(lib, route, "plain", _with_nan_padding(q, QLEN), k, v, QLEN, KVLEN)
    assert torch.equal(_bits(a), _bits(b_))


@pytest.mark.parametrize("form", FORMS)
def test_out_of_range_rows_redo_on_the_exact_path(lib, form):
    """a valid row with a key 150 octaves above the rest (its row sum leaves attn64q's [2^-100, 2^100]): the workgroup redoes its block
    on the exact path — bit for bit attn64p's result — and stays within the bound"""
    q, k, v = _case(seed=17)
    for b, (n, m) in enumerate(zip(QLEN, KVLEN)):
        if m <= 64:              # (one key tile: attn64p's body on both routes)
            continue
        for h in range(H):       # one row per 256-query workgroup: every workgroup of the utterance redoes
            for j, base in enumerate(range(0, n, 256)):   # a score of ~150 (q is pre-scaled: log2 units)
                row = min(base + 40, n - 1)
                qr = q[b, row, h * 64:(h + 1) * 64].double()
                k[b, m - 2 - j, h * 64:(h + 1) * 64] = (qr * (150.0 / float(qr @ qr))).to(torch.bfloat16)
    rin = None if form == "plain" else _resid(form)
    got_q = _run(lib, "attn64q", form, q, k, v, QLEN, KVLEN, resid_in=rin)
    got_p = _run(lib, "attn64p", form, q, k, v, QLEN, KVLEN, resid_in=rin)
    for b, (n, m) in enumerate(zip(QLEN, KVLEN)):
        assert torch.equal(_bits(got_q[b, :n]), _bits(got_p[b, :n])), f"utterance {b}: the redo is not attn64p's exact path"
        o, wabs, s1 = reference(q[b, :n], k[b, :m], v[b, :m], 1, H, n, m, 64)
        want, e = bound(o, wabs, s1, m, 64, None if rin is None else rin[b, :n])
        assert worst_ratio(got_q[b, :n], want, e, stored_bf16=form != "resid_f32") <= 1.0, f"utterance {b}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_bits_do_not_depend_on_neighbours_position_or_padding(lib, route, form):
    """utterance X at position 0 of a batch padded to 600 and at position 2 of a batch padded to 1024 with other neighbours and
    other neighbour lengths: the same bits"""
    n, m = 300, 471
    q1, k1, v1 = _case(seed=21)
    q2, k2, v2 = _case(seed=23, Sq=1024, Skv=1024, Bn=4)
    for src, dst in ((q1, q2), (k1, k2), (v1, v2)):
        dst[2, :src.shape[1]] = src[0]
    ql1, kl1 = [n] + QLEN[1:], [m] + KVLEN[1:]
    ql2, kl2 = [1000, 17, n, 1024], [64, 1024, m, 999]
    r1 = r2 = None
    if form != "plain":
        r1 = _resid(form)
        r2 = _resid(form, Bn=4, Sq=1024, seed=5)
        r2[2, :SQ] = r1[0]
    a = _run(lib, route, form, q1, k1, v1, ql1, kl1, resid_in=r1)
    b_ = _run(lib, route, form, q2, k2, v2, ql2, kl2, resid_in=r2)
    assert torch.equal(_bits(a[0, :n]), _bits(b_[2, :n]))


def test_lengths_are_validated_before_the_launch(lib):
    q, k, v = (x.to(DEV) for x in _case())
    with pytest.raises(ValueError):
        varlen.attention(q, k, v, H, [0] + QLEN[1:], KVLEN)
    with pytest.raises(ValueError):
        varlen.attention(q, k, v, H, QLEN, KVLEN[:-1] + [SKV + 1])
    with pytest.raises(ValueError):
        varlen.attention(q, k, v, H, torch.tensor(QLEN, dtype=torch.float32), KVLEN)
