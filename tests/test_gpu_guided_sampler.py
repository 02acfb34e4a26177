"""SpeechGenerator.sample_guided: the guided strided (DDIM) loop over a variable-length batch.
(a) dense, full lengths, uniform guidance, noises= and cond_by_audio: the bits of the unfused strided chain (forward,
    cfg_combine, linear_update) and of sample_latents_strided;
(b) mixed speech / text / null-text lengths, per-utterance guidance, seeds: each utterance against the fp32 oracle's strided loop on
    its own rows;
(c) padded output rows exactly 0, and NaN in padded rows of the text, the null text and audio_emb changing no bit;
(d) an utterance's latents are the same bits at another position, among other neighbours and with other padding (pinned class);
(e) the refusals."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.around import cfg_combine, linear_update_
from ditto_tts_amd.sampler import SpeechGenerator, strided_schedule
from ditto_tts_amd.synth import hash_normal, synthetic_inputs, synthetic_state_dict
from gpu_util import rel_l2
from oracle import ditto_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS50 = DiTTOConfig(256, 2, 4, 256, 256, 50)


def _model(cfg, seed):
    sd = synthetic_state_dict(cfg, seed)
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


def _nan_pad(x, lens):
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, n:] = float("nan")
    return x


@torch.no_grad()
@pytest.mark.parametrize("cfg_scale", [None, 3.0], ids=["nocfg", "cfg3"])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_dense_is_bitwise_sample_latents_strided(cfg_scale, eta):
    m, _ = _model(STEPS50, 5)
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    B, N, T, S = 2, 64, 32, 25
    text = hash_normal((B, T, 256), "text", 55).to(DEV)
    null = torch.zeros(1, T, 256, device=DEV)
    xinit = hash_normal((B, N, 256), "xT", 55).to(DEV)
    noises = [hash_normal((B, N, 256), f"z{i}", 77) for i in range(S)]
    # the unfused chain per step: forward over [x; x] x [text; null], ditto_cfg_combine, ditto_linear_update
    eng = m.engine()
    x = xinit.clone()
    cond_text = text if cfg_scale is None else torch.cat([text, null.expand_as(text)]).contiguous()
    cond = eng.prepare_text(cond_text, N)
    t = torch.empty(cond_text.shape[0], dtype=torch.long, device=DEV)
    coef = torch.empty(3, B, device=DEV)
    z = torch.empty_like(x)
    for i, (t_val, a, ce, sigma) in enumerate(strided_schedule(sg.alphas_cumprod, S, eta)):
        coef[0].fill_(a); coef[1].fill_(ce); coef[2].fill_(sigma)
        t.fill_(t_val)
        eps = eng.forward(x, cond, t) if cfg_scale is None else cfg_combine(eng.forward(torch.cat([x, x]), cond, t), cfg_scale)
        if sigma != 0.0:
            z.copy_(noises[i].to(DEV))
        linear_update_(x, eps, z if sigma != 0.0 else None, coef[0], coef[1], coef[2])
    want = x
    got = sg.sample_guided(text, xinit, n_steps=S, eta=eta, guidance=cfg_scale, null_text_emb=null, cond_by_audio=True, noises=noises)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want)
    # sample_latents_strided is this loop with one uniform scale
    assert torch.equal(sg.sample_latents_strided(text, xinit, n_steps=S, eta=eta, cfg_scale=cfg_scale, null_text_emb=null,
                                                 cond_by_audio=True, noises=noises), want)
    # guidance as a [B] sequence of one value: the same bits
    if cfg_scale is not None:
        got_v = sg.sample_guided(text, xinit, n_steps=S, eta=eta, guidance=[cfg_scale] * B, null_text_emb=null, cond_by_audio=True,
                                 noises=noises)
        assert torch.equal(got_v, want)


SL, TL, NTL, GUIDE = [64, 23, 41], [32, 9, 20], [5, 32, 12], [5.0, 1.5, 0.0]


@torch.no_grad()
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_varlen_seeded_per_utterance_guidance_against_oracle(eta):
    m, sd = _model(STEPS50, 6)
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    eng = m.engine()
    B, N, T, S = 3, 64, 32, 25
    text = hash_normal((B, T, 256), "text", 8)
    null = hash_normal((B, T, 256), "null", 9) * 0.5
    seeds = torch.tensor([101, 202, 303])
    got = sg.sample_guided(text.to(DEV), torch.zeros(B, N, 256, device=DEV), n_steps=S, eta=eta, guidance=GUIDE,
                           null_text_emb=null.to(DEV), null_text_lengths=NTL, speech_lengths=SL, text_lengths=TL,
                           seeds=seeds.to(DEV)).cpu()
    taus = O.strided_timesteps(50, S)
    worst = 0.0
    for b, (n, k, kn, w) in enumerate(zip(SL, TL, NTL, GUIDE)):
        sb = seeds[b:b + 1].to(DEV)
        xT = eng.noise_normal_(torch.empty(1, N, 256, device=DEV), sb, 0xFFFFFFFF)[:, :n].cpu()
        zs = [eng.noise_normal_(torch.empty(1, N, 256, device=DEV), sb, tau)[:, :n].cpu() for tau in taus]
        want = O.sample_latents_strided(sd, 2, 4, xT, text[b:b + 1, :k], 50, S, noises=zs, eta=eta, cfg_scale=w,
                                        null_text=null[b:b + 1, :kn])
        r = rel_l2(got[b:b + 1, :n], want)
        assert r <= 2e-2, f"utterance {b}: rel-L2 {r:.3e} against the oracle's strided loop"
        worst = max(worst, r)
        assert torch.equal(got[b, n:], torch.zeros_like(got[b, n:])), "padded rows of the latents must be exactly 0"
    print(f"eta {eta}: worst per-utterance rel-L2 against the oracle {worst:.2e}")


@torch.no_grad()
def test_padding_contents_change_no_bit():
    m, _ = _model(STEPS50, 7)
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    B, N, T = 3, 64, 32
    text = hash_normal((B, T, 256), "text", 10)
    null = hash_normal((B, T, 256), "null", 11)
    audio = hash_normal((B, N, 256), "audio", 12)
    noises = [hash_normal((B, N, 256), f"z{i}", 13) for i in range(6)]
    outs = []
    for poison in (False, True):
        t_, n_, a_ = (_nan_pad(text, TL), _nan_pad(null, NTL), _nan_pad(audio, SL)) if poison else (text, null, audio)
        zs = [_nan_pad(z, SL) for z in noises] if poison else noises
        outs.append(sg.sample_guided(t_.to(DEV), a_.to(DEV), n_steps=6, eta=1.0, guidance=GUIDE, null_text_emb=n_.to(DEV),
                                     null_text_lengths=NTL, speech_lengths=SL, text_lengths=TL, cond_by_audio=True,
                                     noises=zs).cpu())
    for b, n in enumerate(SL):
        assert torch.isfinite(outs[0][b, :n]).all()
        assert torch.equal(outs[0][b, n:], torch.zeros_like(outs[0][b, n:]))
    assert torch.equal(outs[0], outs[1]), "NaN in padded rows of text / null text / audio_emb changed a bit"


def _embed(cfg, n, k, Np, Tp, B, pos, seed):
    x1, text1, _ = synthetic_inputs(cfg, 1, n, k, seed=seed)
    x, text, _ = synthetic_inputs(cfg, B, Np, Tp, seed=seed + 100 + Np)
    x[pos, :n], text[pos, :k] = x1[0], text1[0]
    return x, text


@pytest.mark.parametrize("cfg,rows,pads", [(DiTTOConfig(256, 2, 4, 256, 256, 50), 4096, ((1024, 512, 3), (800, 300, 4))),
                                           (DiTTOConfig(768, 2, 12, 256, 768, 50), 17408, ((1024, 512, 2), (768, 300, 3)))],
                         ids=["fp32_stream", "bf16_stream"])
@torch.no_grad()
def test_bits_do_not_depend_on_neighbours_position_or_padding(cfg, rows, pads):
    m, _ = _model(cfg, 1)
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    n, k = 700, 250
    (N1, T1, B1), (N2, T2, B2) = pads
    x1, te1 = _embed(cfg, n, k, N1, T1, B1, 0, 31)
    x2, te2 = _embed(cfg, n, k, N2, T2, B2, 2, 31)
    null1 = hash_normal((1, T1, cfg.text_dim), "null", 3)
    null2 = null1[:, :T2].contiguous()                     # T2 < T1: the utterance's 40 null rows are the same
    SL1, TL1 = [n] + [N1 - 37 * i for i in range(1, B1)], [k] + [T1 - 11 * i for i in range(1, B1)]
    SL2, TL2 = [N2, 129, n] + [65] * (B2 - 3), [T2, 1, k] + [64] * (B2 - 3)
    NL1, NL2 = [40] + [T1] * (B1 - 1), [T2, 3, 40] + [9] * (B2 - 3)
    G1, G2 = [5.0] + [2.0] * (B1 - 1), [0.5, 3.0, 5.0] + [1.0] * (B2 - 3)
    sd1 = torch.tensor([77] + [5 + i for i in range(1, B1)], device=DEV)
    sd2 = torch.tensor([9, 8, 77] + [40 + i for i in range(3, B2)], device=DEV)
    with hip.batch_class(rows):
        if cfg.hidden_dim == 768:
            assert hip.stream_is_bf16(cfg, 2 * B1, N1) and hip.stream_is_bf16(cfg, 2 * B2, N2)
        a = sg.sample_guided(te1.to(DEV), x1.to(DEV), n_steps=3, eta=1.0, guidance=G1, null_text_emb=null1.to(DEV),
                             null_text_lengths=NL1, speech_lengths=SL1, text_lengths=TL1, seeds=sd1).cpu()
        b = sg.sample_guided(te2.to(DEV), x2.to(DEV), n_steps=3, eta=1.0, guidance=G2, null_text_emb=null2.to(DEV),
                             null_text_lengths=NL2, speech_lengths=SL2, text_lengths=TL2, seeds=sd2).cpu()
    assert torch.isfinite(a[0, :n]).all()
    assert torch.equal(a[0, :n], b[2, :n])


@torch.no_grad()
def test_batch_class_argument_pins_the_class():
    """batch_class= gives the bits of the same call under a hip.batch_class scope of (2 with guidance) x batch_class x N rows"""
    cfg = DiTTOConfig(256, 2, 4, 256, 256, 50)
    m, _ = _model(cfg, 2)
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    x, text, _ = synthetic_inputs(cfg, 2, 256, 64, seed=4)
    null = torch.zeros(1, 64, 256)
    kw = dict(n_steps=2, eta=1.0, guidance=[4.0, 2.0], null_text_emb=null.to(DEV), speech_lengths=[256, 100], text_lengths=[64, 30],
              seeds=torch.tensor([1, 2], device=DEV))
    got = sg.sample_guided(text.to(DEV), x.to(DEV), batch_class=16, **kw).cpu()
    with hip.batch_class(2 * 16 * 256):
        want = sg.sample_guided(text.to(DEV), x.to(DEV), **kw).cpu()
    assert torch.equal(got, want)


def test_refusals():
    m, _ = _model(DiTTOConfig(256, 1, 4, 256, 256, 10), 1)
    x, text, _ = synthetic_inputs(DiTTOConfig(256, 1, 4, 256, 256, 10), 2, 96, 40, seed=3)
    x, text = x.to(DEV), text.to(DEV)
    null = torch.zeros(1, 40, 256, device=DEV)
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    with torch.no_grad():
        with pytest.raises(ValueError):
            sg.sample_guided(text, x, n_steps=2, seeds=torch.tensor([1, 2], device=DEV), noises=[x, x])
        with pytest.raises(ValueError):                    # guidance without the unconditional text
            sg.sample_guided(text, x, n_steps=2, guidance=5.0)
        with pytest.raises(ValueError):
            sg.sample_guided(text, x, n_steps=2, guidance=[5.0, 1.0, 2.0], null_text_emb=null)
        with pytest.raises(ValueError):
            sg.sample_guided(text, x, n_steps=2, speech_lengths=[96, 97])
        with pytest.raises(ValueError):
            sg.sample_guided(text, x, n_steps=0)
        wide = DiTTOConfig(256, 1, 2, 256, 256, 10)                 # head_dim 128
        mw, _ = _model(wide, 1)
        with pytest.raises(NotImplementedError):
            SpeechGenerator(ditto_model=mw, device=DEV).sample_guided(text, x, n_steps=2, speech_lengths=[96, 50])
        fp8 = DiTTO(256, 1, 4, 256, 256, 10, fp8_linear=True)
        fp8.load_state_dict(synthetic_state_dict(DiTTOConfig(256, 1, 4, 256, 256, 10), seed=1))
        fp8 = fp8.to(DEV).eval()
        with pytest.raises(NotImplementedError):
            SpeechGenerator(ditto_model=fp8, device=DEV).sample_guided(text, x, n_steps=2, guidance=2.0, null_text_emb=null,
                                                                       text_lengths=[40, 7])
        # the old strided sampler keeps its refusal and points to the new method
        with pytest.raises(NotImplementedError, match="sample_guided"):
            sg.sample_latents_strided(text, x, n_steps=2, speech_lengths=[96, 50])
