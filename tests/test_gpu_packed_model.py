"""Packed batches through the model: DiTTO.forward_packed against the fp32 oracle run per utterance; bit for bit the padded varlen
forward(speech_lengths=, text_lengths=) of the same utterances under the same pinned kernel class (the fp32 stream at d = 256, the
bf16 full-row stream at d = 768); the same bits after permuting the utterances; SpeechGenerator.sample_guided_packed with seeds=
bit for bit sample_guided(seeds=, speech_lengths=, text_lengths=) with guidance off, uniform and per utterance; and the refusals."""
import pytest
import torch

from ditto_tts_amd import hip, varlen
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.synth import hash_normal, synthetic_inputs, synthetic_state_dict
from gpu_util import rel_l2
from oracle import ditto_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = DiTTOConfig(256, 2, 4, 256, 256, 10)
C2L2 = DiTTOConfig(768, 2, 12, 256, 768, 10)
SL, TL = [200, 77, 130, 1, 64], [96, 40, 65, 3, 1]


def _model(cfg, seed=1):
    sd = synthetic_state_dict(cfg, seed=seed)
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


def _packed(x, text, sl, tl):
    xp, cu = varlen.pack(x, sl)
    tp, ct = varlen.pack(text, tl)
    return xp, cu, tp, ct


@pytest.mark.parametrize("cfg,rows", [(SMALL, 4096), (C2L2, 17408)], ids=["d256_fp32_stream", "d768_bf16_stream"])
@torch.no_grad()
def test_forward_packed_against_oracle_and_varlen_bits(cfg, rows):
    m, sd = _model(cfg)
    B = len(SL)
    x, text, t = synthetic_inputs(cfg, B, max(SL), max(TL), seed=5)
    xp, cu, tp, ct = _packed(x, text, SL, TL)
    eps = m.forward_packed(xp.to(DEV), cu, tp.to(DEV), ct, t.to(DEV)).cpu()
    assert eps.shape == xp.shape
    worst = 0.0
    for b, (n, k) in enumerate(zip(SL, TL)):
        want = O.ditto_forward(sd, cfg.num_layers, cfg.num_heads, x[b:b + 1, :n], text[b:b + 1, :k], t[b:b + 1])
        r = rel_l2(eps[int(cu[b]):int(cu[b + 1])].unsqueeze(0), want)
        assert r <= 2e-2, f"utterance {b}: rel-L2 {r:.3e}"
        worst = max(worst, r)
    print(f"d = {cfg.hidden_dim}: worst per-utterance rel-L2 against the oracle {worst:.2e}")
    with hip.batch_class(rows):
        if cfg.hidden_dim == 768:
            assert hip.stream_is_bf16(cfg, B, max(SL))
        pk = m.forward_packed(xp.to(DEV), cu, tp.to(DEV), ct, t.to(DEV)).cpu()
        pad = m(x.to(DEV), text.to(DEV), t.to(DEV), speech_lengths=SL, text_lengths=TL).cpu()
        # the same utterances in reverse order (other offsets, other neighbours, other tile positions)
        perm = list(reversed(range(B)))
        sl2, tl2 = [SL[i] for i in perm], [TL[i] for i in perm]
        xq, cq, tq, ctq = _packed(x[perm], text[perm], sl2, tl2)
        pk2 = m.forward_packed(xq.to(DEV), cq, tq.to(DEV), ctq, t[perm].to(DEV)).cpu()
    for b, n in enumerate(SL):
        seg = pk[int(cu[b]):int(cu[b + 1])]
        assert torch.isfinite(seg).all()
        assert torch.equal(seg, pad[b, :n]), f"utterance {b}: not the padded varlen forward's bits"
        j = perm.index(b)
        assert torch.equal(pk2[int(cq[j]):int(cq[j + 1])], seg), f"utterance {b}: the bits depend on the order"


@torch.no_grad()
@pytest.mark.parametrize("guidance", [None, 3.0, "per"], ids=["nocfg", "uniform", "per_utterance"])
def test_sample_guided_packed_matches_padded_bits(guidance):
    cfg = DiTTOConfig(256, 2, 4, 256, 256, 50)
    m, _ = _model(cfg, seed=4)
    sl, tl = [160, 64, 97, 33], [48, 20, 33, 7]
    B, N, T = len(sl), max(sl), max(tl)
    x, text, _ = synthetic_inputs(cfg, B, N, T, seed=9)
    null = hash_normal((B, T, cfg.text_dim), "null", 3)
    g = [2.0, 3.0, 4.5, 1.0] if guidance == "per" else guidance
    seeds = torch.tensor([11, 12, 13, 14], device=DEV)
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    kw = dict(n_steps=4, eta=1.0, guidance=g, seeds=seeds, batch_class=B)
    if g is not None:
        kw["null_text_emb"] = null.to(DEV)
    pad = sg.sample_guided(text.to(DEV), x.to(DEV), speech_lengths=sl, text_lengths=tl, **kw).cpu()
    xp, cu, tp, ct = _packed(x, text, sl, tl)
    if g is not None:
        kw["null_text_emb"] = varlen.pack(null, tl)[0].to(DEV)
    got = sg.sample_guided_packed(tp.to(DEV), ct, xp.to(DEV), cu, **kw).cpu()
    assert got.shape == xp.shape
    for b, n in enumerate(sl):
        seg = got[int(cu[b]):int(cu[b + 1])]
        assert torch.isfinite(seg).all()
        assert torch.equal(seg, pad[b, :n]), f"utterance {b}: not sample_guided's bits"


def test_refusals():
    m, _ = _model(SMALL)
    x, text, t = synthetic_inputs(SMALL, 2, 96, 40, seed=3)
    xp, cu, tp, ct = _packed(x, text, [96, 50], [40, 7])
    xp, tp, t = xp.to(DEV), tp.to(DEV), t.to(DEV)
    with pytest.raises(NotImplementedError):          # autograd (training): parameters require grad, grad enabled
        m.forward_packed(xp, cu, tp, ct, t)
    with torch.no_grad():
        with pytest.raises(ValueError):
            m.forward_packed(xp, [0, 96, 147], tp, ct, t)         # last offset != rows
        with pytest.raises(ValueError):
            m.forward_packed(xp, cu, tp, [0, 40, 40], t)           # an empty utterance
        wide = DiTTOConfig(256, 1, 2, 256, 256, 10)                # head_dim 128
        mw, _ = _model(wide)
        with pytest.raises(NotImplementedError):
            mw.forward_packed(xp, cu, tp, ct, t)
        with pytest.raises(NotImplementedError):
            SpeechGenerator(ditto_model=mw, device=DEV).sample_guided_packed(tp, ct, xp, cu, n_steps=2)
        fp8 = DiTTO(256, 1, 4, 256, 256, 10, fp8_linear=True)
        fp8.load_state_dict(synthetic_state_dict(DiTTOConfig(256, 1, 4, 256, 256, 10), seed=1))
        fp8 = fp8.to(DEV).eval()
        with pytest.raises(NotImplementedError):
            fp8.forward_packed(xp, cu, tp, ct, t)
