"""Variable-length batches through the model: DiTTO.forward(x, text_emb, t, speech_lengths=, text_lengths=) against the fp32 oracle
run per utterance at its own (N_b, T_b); padded eps rows exactly 0; NaN padding changes nothing; an utterance's bits do not depend on
its neighbours, its position or the padded lengths under a pinned kernel class (fp32 stream; d = 768 bf16 full-row stream); the
seeded ancestral loop against each utterance's solo loop; and the refusals."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.synth import synthetic_inputs, synthetic_state_dict
from gpu_util import rel_l2
from oracle import ditto_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = DiTTOConfig(256, 2, 4, 256, 256, 10)
C2L2 = DiTTOConfig(768, 2, 12, 256, 768, 10)


def _model(cfg, seed=1):
    sd = synthetic_state_dict(cfg, seed=seed)
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


def _nan_pad(x, lens):
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, n:] = float("nan")
    return x


@pytest.mark.parametrize("cfg", [SMALL, C2L2], ids=["d256", "d768"])
@torch.no_grad()
def test_forward_against_oracle_per_utterance(cfg):
    m, sd = _model(cfg)
    SL, TL = [200, 77, 130], [96, 40, 65]
    x, text, t = synthetic_inputs(cfg, 3, 200, 96, seed=5)
    eps = m(x.to(DEV), text.to(DEV), t.to(DEV), speech_lengths=SL, text_lengths=TL).cpu()
    worst = 0.0
    for b, (n, k) in enumerate(zip(SL, TL)):
        want = O.ditto_forward(sd, cfg.num_layers, cfg.num_heads, x[b:b + 1, :n], text[b:b + 1, :k], t[b:b + 1])
        r = rel_l2(eps[b:b + 1, :n], want)
        assert r <= 2e-2, f"utterance {b}: rel-L2 {r:.3e}"
        worst = max(worst, r)
        assert torch.equal(eps[b, n:], torch.zeros_like(eps[b, n:])), "padded eps rows must be exactly 0"
    print(f"d = {cfg.hidden_dim}: worst per-utterance rel-L2 against the oracle {worst:.2e}")
    # NaN in every padding row of x and text_emb changes no bit
    eps_nan = m(_nan_pad(x, SL).to(DEV), _nan_pad(text, TL).to(DEV), t.to(DEV), speech_lengths=SL, text_lengths=TL).cpu()
    assert torch.equal(eps_nan, eps)
    # full lengths: within tolerance of the dense call (another attention kernel family: not bit for bit)
    dense = m(x.to(DEV), text.to(DEV), t.to(DEV)).cpu()
    full = m(x.to(DEV), text.to(DEV), t.to(DEV), speech_lengths=torch.tensor([200] * 3), text_lengths=(96, 96, 96)).cpu()
    assert rel_l2(full, dense) < 1e-2


def _embed(cfg, n, k, Np, Tp, B, pos, seed):
    """a batch of B utterances padded to (Np, Tp) with the utterance (x, text, t) of `seed` at `pos` and other neighbours"""
    x1, text1, t1 = synthetic_inputs(cfg, 1, n, k, seed=seed)
    x, text, t = synthetic_inputs(cfg, B, Np, Tp, seed=seed + 100 + Np)
    x[pos, :n], text[pos, :k], t[pos] = x1[0], text1[0], t1[0]
    return x, text, t


@pytest.mark.parametrize("cfg,rows,pads", [(SMALL, 4096, ((1024, 512, 3), (800, 300, 4))),
                                           (C2L2, 17408, ((1024, 512, 2), (768, 300, 3)))], ids=["fp32_stream", "bf16_stream"])
@torch.no_grad()
def test_bits_do_not_depend_on_neighbours_position_or_padding(cfg, rows, pads):
    m, _ = _model(cfg)
    n, k = 700, 250
    (N1, T1, B1), (N2, T2, B2) = pads
    x1, te1, t1 = _embed(cfg, n, k, N1, T1, B1, 0, 31)
    x2, te2, t2 = _embed(cfg, n, k, N2, T2, B2, 2, 31)
    SL1, TL1 = [n] + [N1 - 37 * i for i in range(1, B1)], [k] + [T1 - 11 * i for i in range(1, B1)]
    SL2, TL2 = [N2, 129, n] + [65] * (B2 - 3), [T2, 1, k] + [64] * (B2 - 3)
    with hip.batch_class(rows):
        if cfg.hidden_dim == 768:
            assert hip.stream_is_bf16(cfg, B1, N1) and hip.stream_is_bf16(cfg, B2, N2)
        a = m(x1.to(DEV), te1.to(DEV), t1.to(DEV), speech_lengths=SL1, text_lengths=TL1).cpu()
        b = m(x2.to(DEV), te2.to(DEV), t2.to(DEV), speech_lengths=SL2, text_lengths=TL2).cpu()
    assert torch.isfinite(a[0, :n]).all()
    assert torch.equal(a[0, :n], b[2, :n])


@torch.no_grad()
def test_seeded_loop_matches_solo_loops():
    cfg = SMALL
    m, _ = _model(cfg, seed=3)
    SL, TL = [160, 64, 97], [48, 20, 33]
    x, text, _ = synthetic_inputs(cfg, 3, 160, 48, seed=9)
    seeds = torch.tensor([11, 12, 13])
    sg = SpeechGenerator(ditto_model=m, device=DEV)
    got = sg.sample_latents(text.to(DEV), x.to(DEV), seeds=seeds.to(DEV), speech_lengths=SL, text_lengths=TL).cpu()
    for b, (n, k) in enumerate(zip(SL, TL)):
        solo = sg.sample_latents(text[b:b + 1, :k].contiguous().to(DEV), x[b:b + 1, :n].contiguous().to(DEV),
                                 seeds=seeds[b:b + 1].to(DEV)).cpu()
        r = rel_l2(got[b:b + 1, :n], solo)
        assert r <= 2e-2, f"utterance {b}: rel-L2 {r:.3e} against its solo seeded loop"
        assert torch.equal(got[b, n:], torch.zeros_like(got[b, n:])), "padded rows of the latents must be 0"
    # the noises= path: padded rows 0 as well
    zs = [torch.randn(3, 160, cfg.hidden_dim) for _ in range(sg._loop_steps())]
    got_n = sg.sample_latents(text.to(DEV), x.to(DEV), noises=zs, speech_lengths=SL, text_lengths=TL).cpu()
    for b, n in enumerate(SL):
        assert torch.isfinite(got_n[b, :n]).all() and torch.equal(got_n[b, n:], torch.zeros_like(got_n[b, n:]))


def test_refusals():
    m, _ = _model(SMALL)
    x, text, t = synthetic_inputs(SMALL, 2, 96, 40, seed=3)
    x, text, t = x.to(DEV), text.to(DEV), t.to(DEV)
    with pytest.raises(NotImplementedError):          # autograd (training): parameters require grad, grad enabled
        m(x, text, t, speech_lengths=[96, 50])
    with torch.no_grad():
        with pytest.raises(ValueError):
            m(x, text, t, speech_lengths=[96, 97])
        with pytest.raises(ValueError):
            m(x, text, t, text_lengths=[0, 3])
        sg = SpeechGenerator(ditto_model=m, device=DEV)
        with pytest.raises(NotImplementedError):
            sg.sample_latents_strided(text, x, n_steps=2, speech_lengths=[96, 50])
        from ditto_tts_amd import dist
        with pytest.raises(NotImplementedError):
            dist.sample_sharded(lambda *a: None, text, x, None, None, DEV, speech_lengths=[96, 50])
        wide = DiTTOConfig(256, 1, 2, 256, 256, 10)                 # head_dim 128
        mw, _ = _model(wide)
        with pytest.raises(NotImplementedError):
            mw(x, text, t, speech_lengths=[96, 50])
        fp8 = DiTTO(256, 1, 4, 256, 256, 10, fp8_linear=True)
        fp8.load_state_dict(synthetic_state_dict(DiTTOConfig(256, 1, 4, 256, 256, 10), seed=1))
        fp8 = fp8.to(DEV).eval()
        with pytest.raises(NotImplementedError):
            fp8(x, text, t, speech_lengths=[96, 50])
