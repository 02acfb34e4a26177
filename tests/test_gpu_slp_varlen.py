"""-m gpu: variable-length batches of the speech-length predictor.

(a) the last-row attention kernel against fp64 torch on the bf16-rounded operands, elementwise;
(b) the GEMM-composed attention with lengths (ditto_attention_causal_varlen_bf16) per utterance against its own slice;
(c) the stack: every utterance of a padded batch against oracle.slp_decode on its own slice, and the bitwise properties
    (padding contents, batch order, repetition) that make a batch equal to one call per utterance.

The off-by-one in a key count is held by (a) and (b): their last valid key carries most of the probability mass and the
rows behind it are NaN.  The stack test sees a wrong ROW (len - 2 for len - 1 moves the logits by >= 0.19 rel-L2) but one
text key too few moves them by only 2.6e-2 .. 5.7e-2, too close to the 2e-2 tolerance to be relied on."""
import ctypes as C
import functools
import math

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.slp import SLP
from ditto_tts_amd.synth import hash_normal, synthetic_slp_state_dict
from gpu_util import asym, bf16, rel_l2, stream
from oracle import ditto_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2          # the project's stated SLP tolerance (tests/test_gpu_slp.py)
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip.lib()


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ (a) last-row attention
LR_SKV = 300


def _lr_case(B, H, dh, lens, seed):
    """q [B, ldq], k / v [B * Skv, ld] bf16 with NaN in every row at or past the length and in the columns past H * dh;
    the last valid key aligned with q so that it carries most of the mass, its value row distinct."""
    D, ld = H * dh, H * dh + 64
    q = torch.full((B, ld), NAN)
    q[:, :D] = asym((B, D), seed)
    k = torch.full((B, LR_SKV, ld), NAN)
    v = torch.full((B, LR_SKV, ld), NAN)
    kk, vv = asym((B, LR_SKV, D), seed + 1), asym((B, LR_SKV, D), seed + 2)
    for b, L in enumerate(lens):
        k[b, :L, :D], v[b, :L, :D] = kk[b, :L], vv[b, :L]
        for h in range(H):
            qh = q[b, h * dh:(h + 1) * dh]
            # score of the last key = ln(L) + 3 after the 1/sqrt(dh) scale: about e^3 times the mass of all the others
            k[b, L - 1, h * dh:(h + 1) * dh] = qh * ((math.log(L) + 3.0) * math.sqrt(dh) / float(qh @ qh))
        v[b, L - 1, :D] = 2.5 + 0.5 * vv[b, L - 1]
    return bf16(q.to(DEV)), bf16(k.view(B * LR_SKV, ld).to(DEV)), bf16(v.view(B * LR_SKV, ld).to(DEV)), ld


def _lr_want(q, k, v, B, H, dh, lens, scale):
    """fp64 on the bf16-rounded operands: the output and the bound's sum_j p_j |v_j|, and the output without the last key"""
    ld = q.shape[1]
    kd, vd = k.double().view(B, LR_SKV, ld), v.double().view(B, LR_SKV, ld)
    want = torch.zeros(B, H * dh, dtype=torch.float64, device=DEV)
    mag, drop = torch.zeros_like(want), torch.zeros_like(want)
    for b, L in enumerate(lens):
        for h in range(H):
            c = slice(h * dh, (h + 1) * dh)
            s = (kd[b, :L, c] @ q[b, c].double()) * scale
            p = torch.softmax(s, 0)
            want[b, c], mag[b, c] = p @ vd[b, :L, c], p @ vd[b, :L, c].abs()
            if L > 1:
                drop[b, c] = torch.softmax(s[:L - 1], 0) @ vd[b, :L - 1, c]
    return want, mag, drop


@pytest.mark.parametrize("B,H,dh", [(2, 4, 64), (1, 1, 192), (2, 4, 384), (1, 1, 1472)])
def test_last_row_attention(lib, B, H, dh):
    """|out - want| <= 2^-8 sum_j p_j |v_j| elementwise: the bound the feature was specified with, derived from the formats and
    not fitted.  Its margin is smaller than a factor of two, though: round-to-nearest to bf16's 8 significant bits errs by up to
    2^-8 / (1 + 2^-8) of |result| (a value just above a power of two), and with one dominant key and same-signed values
    |result| is nearly the whole sum.  What is left for the arithmetic is what the kernel needs: fp32 accumulation over <= 2048
    keys and the v_exp error stay below 2^-12 of the sum.  Measured on an MI355X: worst ratio 0.968 (dh 1472, length 64),
    0.82 .. 0.97 over all shapes and lengths; inputs and kernel are deterministic, so these figures repeat."""
    chunk = hip.get_option("slp_lr_chunk")
    assert 1 < chunk < LR_SKV - 1, "the lengths below sit on the chunk boundaries"
    all_lens = [1, 63, 64, 65, LR_SKV, chunk - 1, chunk, chunk + 1]
    D, scale = H * dh, 1.0 / math.sqrt(dh)
    nb = lib.ditto_attention_last_row_workspace_bytes(B, H, LR_SKV, dh)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    worst = 0.0
    for i in range(0, len(all_lens), B):
        lens = all_lens[i:i + B]
        lens_d = i32(lens)
        q, k, v, ld = _lr_case(B, H, dh, lens, 40 + i)
        want, mag, drop = _lr_want(q, k, v, B, H, dh, lens, scale)
        # the output: a window of a sentinel buffer, rows at a stride wider than the row
        ldo, off = D + 64, 3 * ld + 8
        outs = []
        for _ in range(2):
            buf = torch.full((off + B * ldo + 512,), 777.0, dtype=torch.bfloat16, device=DEV)
            win = buf[off:off + B * ldo].view(B, ldo)
            hip.check(lib.ditto_attention_last_row_bf16(q.data_ptr(), ld, k.data_ptr(), ld, v.data_ptr(), ld, win.data_ptr(),
                                                        ldo, lens_d.data_ptr(), B, H, LR_SKV, dh, scale, ws.data_ptr(), nb,
                                                        stream()))
            torch.cuda.synchronize()
            outs.append(buf)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two runs differ"
        buf = outs[0]
        win = buf[off:off + B * ldo].view(B, ldo)
        assert bool((buf[:off] == 777.0).all()) and bool((buf[off + B * ldo:] == 777.0).all())
        assert bool((win[:, D:] == 777.0).all()), "written outside the window"
        out = win[:, :D].double()
        assert bool(torch.isfinite(out).all()), f"NaN from the rows past the length, lens {lens}"
        ratio = float(((out - want).abs() / (2.0 ** -8 * mag)).max())
        worst = max(worst, ratio)
        print(f"last_row B{B} H{H} dh{dh} lens {lens}: worst |err| / bound = {ratio:.3f}")
        assert ratio <= 1.0, f"lens {lens}: {ratio}"
        for b, L in enumerate(lens):                      # the case is sharp: without the last key the output moves by O(1)
            if L > 1:
                assert float((drop[b] - want[b]).abs().mean()) > 0.5
    print(f"last_row B{B} H{H} dh{dh}: worst ratio over all lengths {worst:.3f}")
    # len NULL = all Skv rows; refusals
    q, k, v, ld = _lr_case(B, H, dh, [LR_SKV] * B, 77)
    a = torch.empty(B, D, dtype=torch.bfloat16, device=DEV)
    b_ = torch.empty_like(a)
    hip.check(lib.ditto_attention_last_row_bf16(q.data_ptr(), ld, k.data_ptr(), ld, v.data_ptr(), ld, a.data_ptr(), D, None, B, H,
                                                LR_SKV, dh, scale, ws.data_ptr(), nb, stream()))
    lens_d = i32([LR_SKV] * B)
    hip.check(lib.ditto_attention_last_row_bf16(q.data_ptr(), ld, k.data_ptr(), ld, v.data_ptr(), ld, b_.data_ptr(), D,
                                                lens_d.data_ptr(), B, H, LR_SKV, dh, scale, ws.data_ptr(), nb,
                                                stream()))
    assert torch.equal(a, b_)
    assert lib.ditto_attention_last_row_bf16(q.data_ptr(), ld, k.data_ptr(), ld, v.data_ptr(), ld, a.data_ptr(), D, None, B, H,
                                             LR_SKV, dh, scale, ws.data_ptr(), nb - 1, stream()) == hip.ERR_SIZE
    assert lib.ditto_attention_last_row_bf16(q.data_ptr(), ld + 4, k.data_ptr(), ld, v.data_ptr(), ld, a.data_ptr(), D, None, B,
                                             H, LR_SKV, dh, scale, ws.data_ptr(), nb, stream()) == hip.ERR_SHAPE
    assert lib.ditto_attention_last_row_workspace_bytes(1, 1, 8, 96) == 0


# ------------------------------------------------------------------ (b) the composed path with lengths
def _attn_slice(q, k, v, H, dh, scale, causal):
    """fp32 attention of ONE utterance: q [Sq, H*dh], k / v [Skv, H*dh]; causal aligned to the end of the keys"""
    Sq, Skv = q.shape[0], k.shape[0]
    qh, kh, vh = (t.float().view(-1, H, dh).transpose(0, 1) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        i = torch.arange(Sq, device=q.device)[:, None]
        j = torch.arange(Skv, device=q.device)[None, :]
        s = s.masked_fill(j > i + (Skv - Sq), float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(Sq, H * dh)


@pytest.mark.parametrize("B,H,Sq,Skv,dh,causal,q_len,kv_len", [
    (2, 4, 40, 40, 64, True, [40, 1], [40, 1]),
    (2, 4, 130, 130, 384, True, [65, 130], [65, 130]),
    (3, 2, 33, 70, 64, False, [33, 5, 20], [70, 1, 33]),
    (3, 2, 33, 70, 64, False, None, [64, 65, 70]),
])
def test_composed_attention_with_lengths(lib, B, H, Sq, Skv, dh, causal, q_len, kv_len):
    D = H * dh
    scale = 1.0 / math.sqrt(dh)
    q0, k0, v0 = asym((B, Sq, D), 21), asym((B, Skv, D), 22), asym((B, Skv, D), 23)
    ql = q_len if q_len is not None else [Sq] * B
    nb = lib.ditto_attention_causal_workspace_bytes(B, H, Sq, Skv, dh)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    qld, kld = (None if q_len is None else i32(q_len)), i32(kv_len)   # kept alive: the call only takes their addresses
    outs = []
    for fill in (0.37, NAN):                       # finite padding, then NaN in every padded q / k / v row
        q, k, v = q0.clone(), k0.clone(), v0.clone()
        for b in range(B):
            q[b, ql[b]:], k[b, kv_len[b]:], v[b, kv_len[b]:] = fill, fill, fill
        q, k, v = (bf16(t.view(-1, D).to(DEV)) for t in (q, k, v))
        out = torch.full((B * Sq, D), 777.0, dtype=torch.bfloat16, device=DEV)
        hip.check(lib.ditto_attention_causal_varlen_bf16(
            q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D,
            None if q_len is None else qld.data_ptr(), kld.data_ptr(), B, H, Sq, Skv, dh, scale, int(causal),
            ws.data_ptr(), nb, stream()))
        outs.append(out.view(B, Sq, D))
    worst = 0.0
    for b in range(B):
        qb, kb, vb = (bf16(t[b, :n].to(DEV)) for t, n in ((q0, ql[b]), (k0, kv_len[b]), (v0, kv_len[b])))
        want = _attn_slice(qb, kb, vb, H, dh, scale, causal)
        for out in outs:
            got = out[b, :ql[b]]
            assert bool(torch.isfinite(got.float()).all()), f"utterance {b}: the padding reached a valid row"
            worst = max(worst, rel_l2(got.float(), want))
            assert bool((out[b, ql[b]:] == 0).all()), "query rows past the length must be zero"
        assert torch.equal(outs[0][b, :ql[b]].view(torch.int16), outs[1][b, :ql[b]].view(torch.int16)), \
            f"utterance {b}: NaN padding changed valid rows"
    print(f"composed varlen B{B} H{H} {Sq}x{Skv} dh{dh}: worst rel_l2 per utterance {worst:.2e}")
    assert worst < 8e-3                            # the figure of test_gpu_slp.py::test_causal_attention
    assert lib.ditto_attention_causal_varlen_bf16(q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D, None,
                                                  None, B, H, Sq, Skv, dh, scale, int(causal), ws.data_ptr(), nb - 1,
                                                  stream()) == hip.ERR_SIZE


# ------------------------------------------------------------------ (c) the stack
NCLS = 11
STACK = {
    "d128_h4_l2": (128, 4, 2, 6, 200, 40, [1, 37, 64, 65, 129, 200], [40, 1, 7, 33, 17, 5]),
    "d192_h1_l1": (192, 1, 1, 6, 200, 40, [1, 37, 64, 65, 129, 200], [40, 1, 7, 33, 17, 5]),
    "d256_h2_l3": (256, 2, 3, 6, 200, 40, [1, 37, 64, 65, 129, 200], [40, 1, 7, 33, 17, 5]),
    "d1472_h4_l4": (1472, 4, 4, 3, 96, 32, [96, 1, 65], [32, 1, 17]),
}


@functools.lru_cache(maxsize=None)
def _stack_case(name):
    """model, inputs and the oracle's per-utterance answers (computed once per config, on the CPU, never modified)"""
    d, nhead, nl, B, S, T, alen, tlen = STACK[name]
    sd = synthetic_slp_state_dict(d, nhead, nl, NCLS, 3)
    m = SLP(NCLS, nhead, nl, hidden_size=d)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    z_text, z_audio = hash_normal((B, T, d), "t", 3), hash_normal((B, S, d), "a", 3)
    want = [O.slp_decode(sd, nl, nhead, z_text[b:b + 1, :tlen[b]], z_audio[b:b + 1, :alen[b]]) for b in range(B)]
    want_full_text = [O.slp_decode(sd, nl, nhead, z_text[b:b + 1], z_audio[b:b + 1, :alen[b]])[0] for b in range(B)]
    want_full_audio = [O.slp_decode(sd, nl, nhead, z_text[b:b + 1, :tlen[b]], z_audio[b:b + 1])[0] for b in range(B)]
    return m, sd, z_text, z_audio, want, want_full_text, want_full_audio


def _padded(z, lens, fill, seed=9):
    """z with everything at or past the lengths replaced: a number, or "other" = large finite values"""
    z = z.clone()
    other = 1e3 * hash_normal(tuple(z.shape), "pad", seed) if fill == "other" else None
    for b, n in enumerate(lens):
        z[b, n:] = other[b, n:] if other is not None else fill
    return z.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", sorted(STACK))
def test_stack_matches_oracle_per_utterance(name):
    d, nhead, nl, B, S, T, alen, tlen = STACK[name]
    m, sd, z_text, z_audio, want, _, _ = _stack_case(name)
    zt, za = _padded(z_text, tlen, NAN), _padded(z_audio, alen, NAN)
    logits_lr = m.decode(zt, za, audio_lengths=alen, text_lengths=tlen)               # last layer on the last rows
    logits, dec = m.decode(zt, za, return_decoded=True, audio_lengths=alen, text_lengths=torch.tensor(tlen))
    assert logits.shape == (B, NCLS) and dec.shape == (B, S, d) and logits_lr.shape == (B, NCLS)
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        wl, wd = want[b]
        e = (rel_l2(logits_lr[b], wl[0]), rel_l2(logits[b], wl[0]), rel_l2(dec[b, :alen[b]], wd[0]))
        worst = [max(a, c) for a, c in zip(worst, e)]
        assert bool((dec[b, alen[b]:] == 0).all()), f"utterance {b}: decoded rows past the length are not exactly 0"
    print(f"{name}: worst rel_l2 logits (last-row path) {worst[0]:.2e}, logits (full path) {worst[1]:.2e}, "
          f"decoded {worst[2]:.2e}")
    assert max(worst) <= TOL
    assert torch.equal(m.predict_class(zt, za, audio_lengths=alen, text_lengths=tlen), logits_lr.argmax(-1))


@pytest.mark.parametrize("name", sorted(STACK))
def test_stack_padding_order_and_repetition_are_bitwise(name):
    d, nhead, nl, B, S, T, alen, tlen = STACK[name]
    m, sd, z_text, z_audio, _, _, _ = _stack_case(name)
    ref = None
    for fill in (0.0, NAN, "other", 0.0):          # the last one: a second run of the first
        zt, za = _padded(z_text, tlen, fill), _padded(z_audio, alen, fill)
        lr = m.decode(zt, za, audio_lengths=alen, text_lengths=tlen)
        logits, dec = m.decode(zt, za, return_decoded=True, audio_lengths=alen, text_lengths=tlen)
        got = (lr, logits, [dec[b, :alen[b]].clone() for b in range(B)])
        if ref is None:
            ref = got
            continue
        assert torch.equal(_bits(got[0]), _bits(ref[0])), f"padding {fill}: last-row logits changed"
        assert torch.equal(_bits(got[1]), _bits(ref[1])), f"padding {fill}: logits changed"
        for b in range(B):
            assert torch.equal(_bits(got[2][b]), _bits(ref[2][b])), f"padding {fill}: decoded rows of utterance {b} changed"
    # the batch in reversed order: every utterance keeps its own bits
    zt, za = _padded(z_text, tlen, NAN).flip(0), _padded(z_audio, alen, NAN).flip(0)
    ra, rt = alen[::-1], tlen[::-1]
    lr = m.decode(zt, za, audio_lengths=ra, text_lengths=rt)
    logits, dec = m.decode(zt, za, return_decoded=True, audio_lengths=ra, text_lengths=rt)
    assert torch.equal(_bits(lr.flip(0)), _bits(ref[0])) and torch.equal(_bits(logits.flip(0)), _bits(ref[1]))
    for b in range(B):
        assert torch.equal(_bits(dec[B - 1 - b, :alen[b]]), _bits(ref[2][b])), f"reversed batch: utterance {b}"


@pytest.mark.parametrize("name", sorted(STACK))
def test_last_row_path_against_full_path(name):
    """slp_last_row = 0 (every layer composed) against 1 (the default): both hold the tolerance against the oracle.  Their direct
    difference is printed, not asserted: the two paths round differently (GEMMs at M = B against M = B S, flash-style partial
    sums against bf16 probabilities) and nothing but the oracle says which is closer."""
    d, nhead, nl, B, S, T, alen, tlen = STACK[name]
    m, sd, z_text, z_audio, want, _, _ = _stack_case(name)
    zt, za = _padded(z_text, tlen, NAN), _padded(z_audio, alen, NAN)
    assert hip.get_option("slp_last_row") == 1
    on = m.decode(zt, za, audio_lengths=alen, text_lengths=tlen)
    try:
        hip.set_option("slp_last_row", 0)
        off = m.decode(zt, za, audio_lengths=alen, text_lengths=tlen)
    finally:
        hip.set_option("slp_last_row", 1)
    full, _ = m.decode(zt, za, return_decoded=True, audio_lengths=alen, text_lengths=tlen)
    assert torch.equal(_bits(off), _bits(full))     # without the last-row path, asking for `decoded` changes nothing
    e_on = max(rel_l2(on[b], want[b][0][0]) for b in range(B))
    e_off = max(rel_l2(off[b], want[b][0][0]) for b in range(B))
    direct = max(rel_l2(on[b], off[b]) for b in range(B))
    print(f"{name}: last-row path {e_on:.2e}, full path {e_off:.2e} against the oracle; last-row against full {direct:.2e}")
    assert e_on <= TOL and e_off <= TOL
    with pytest.raises(hip.DittoHipError):
        hip.set_option("slp_last_row", 2)
    assert hip.get_option("slp_last_row") == 1


@pytest.mark.parametrize("name", ["d128_h4_l2", "d192_h1_l1"])
def test_lengths_given_alone(name):
    """audio_lengths alone: every text row counts; text_lengths alone: every audio row, so the logits come from row S - 1."""
    d, nhead, nl, B, S, T, alen, tlen = STACK[name]
    m, sd, z_text, z_audio, _, want_full_text, want_full_audio = _stack_case(name)
    zt, za = z_text.to(DEV), _padded(z_audio, alen, NAN)
    for dec in (False, True):
        a = m.decode(zt, za, dec, audio_lengths=alen)
        b_ = m.decode(zt, za, dec, audio_lengths=alen, text_lengths=[T] * B)
        a, b_ = (a[0], b_[0]) if dec else (a, b_)
        assert torch.equal(_bits(a), _bits(b_))
        assert max(rel_l2(a[b], want_full_text[b][0]) for b in range(B)) <= TOL
    zt, za = _padded(z_text, tlen, NAN), z_audio.to(DEV)
    for dec in (False, True):
        a = m.decode(zt, za, dec, text_lengths=tlen)
        b_ = m.decode(zt, za, dec, audio_lengths=[S] * B, text_lengths=tlen)
        a, b_ = (a[0], b_[0]) if dec else (a, b_)
        assert torch.equal(_bits(a), _bits(b_))
        assert max(rel_l2(a[b], want_full_audio[b][0]) for b in range(B)) <= TOL


def test_dense_entry_is_untouched_by_the_keywords():
    """No lengths: the dense entry, bit for bit what the positional call gives; full lengths agree with it to the tolerance."""
    d, nhead, nl, B, S, T, alen, tlen = STACK["d128_h4_l2"]
    m, sd, z_text, z_audio, _, _, _ = _stack_case("d128_h4_l2")
    zt, za = z_text.to(DEV), z_audio.to(DEV)
    a = m.decode(zt, za)
    b_ = m.decode(zt, za, audio_lengths=None, text_lengths=None)
    assert torch.equal(_bits(a), _bits(b_))
    full = m.decode(zt, za, audio_lengths=[S] * B, text_lengths=[T] * B)
    assert rel_l2(full, a) <= TOL
    lib = hip.lib()
    cfg = hip.SlpConfig(d, nhead, nl, d * nhead, NCLS)
    assert lib.ditto_slp_varlen_workspace_bytes(C.byref(cfg), B, S, T) > lib.ditto_slp_workspace_bytes(C.byref(cfg), B, S, T)
    assert lib.ditto_slp_varlen_workspace_bytes(C.byref(cfg), 0, S, T) == 0
    assert lib.ditto_slp_forward_varlen(None, None, None, None, None, 1, 1, 1, None, None, None, 0, None) == hip.ERR_ARG
