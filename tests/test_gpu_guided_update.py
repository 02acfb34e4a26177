"""The fused guided update alone (ditto_guided_update, csrc/guided.hip): on every valid row bitwise equal to the chain it replaces
(cfg_combine + linear_update, with the noise from a buffer or from ditto_noise_normal), padded rows exactly 0 in both halves, both
halves equal, and NaN in the padded rows of x / eps2 / the noise buffer changing no bit."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.around import cfg_combine, guided_update_, linear_update_
from ditto_tts_amd.synth import hash_normal
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _noise_normal(B, N, d, seeds, step):
    z = torch.empty(B, N, d, device=DEV)
    hip.check(hip.lib().ditto_noise_normal(z.data_ptr(), seeds.data_ptr(), step & 0xFFFFFFFF, B, N * d, stream()))
    return z


def _old_chain(x, eps2, z, a, ce, cz, w_uniform, cfg):
    """the strided sampler's chain: cfg_combine (one scale), then linear_update (z None: no noise term)"""
    eps = cfg_combine(eps2, w_uniform) if cfg else eps2.clone()
    out = x.clone()
    linear_update_(out, eps, z, a, ce, cz)
    return out


CASES = [(B, N, d) for B, N, d in [(1, 1, 256), (3, 65, 768), (7, 1000, 256), (3, 1000, 768), (7, 65, 256), (1, 1000, 768)]]


@pytest.mark.parametrize("B,N,d", CASES, ids=[f"B{B}_N{N}_d{d}" for B, N, d in CASES])
@pytest.mark.parametrize("mode", ["none", "buffer", "philox"])
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
def test_bitwise_equal_to_the_old_chain(B, N, d, mode, cfg):
    nb = 2 * B if cfg else B
    x = hash_normal((B, N, d), "x", B * N + d).to(DEV)
    eps2 = hash_normal((nb, N, d), "e", B + N + d).to(DEV)
    a = torch.linspace(0.9, 1.1, B, device=DEV)
    ce = torch.linspace(-0.4, 0.05, B, device=DEV)
    cz = torch.linspace(0.0, 0.3, B, device=DEV) + (0.0 if mode == "none" else 0.01)
    seeds = torch.arange(B, device=DEV, dtype=torch.long) * 7919 + 3
    step = 37
    w_val = 3.0
    w = torch.full((B,), w_val, device=DEV)
    noise = hash_normal((B, N, d), "z", N).to(DEV) if mode == "buffer" else None
    z = noise if mode == "buffer" else (_noise_normal(B, N, d, seeds, step) if mode == "philox" else None)
    want = _old_chain(x, eps2, z, a, ce, cz if mode != "none" else torch.zeros_like(cz), w_val, cfg)

    # dense (speech_len NULL)
    x2 = torch.cat([x, x]) if cfg else x.clone()
    guided_update_(x2, eps2, a, ce, cz, w=w if cfg else None, noise=noise, seeds=seeds if mode == "philox" else None, step=step)
    assert torch.equal(x2[:B], want)
    if cfg:
        assert torch.equal(x2[B:], want)

    # ragged lengths: valid rows as above, padded rows 0 in both halves, NaN padding changes nothing
    lens = [max(1, (N * (b + 1)) // B - b) for b in range(B)]
    lens[0] = N if B > 1 else lens[0]
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    results = []
    for poison in (False, True):
        xp, ep = x.clone(), eps2.clone()
        zp = noise.clone() if noise is not None else None
        if poison:
            for b, n in enumerate(lens):
                xp[b, n:] = float("nan")
                ep[b, n:] = float("nan")
                if cfg:
                    ep[B + b, n:] = float("nan")
                if zp is not None:
                    zp[b, n:] = float("nan")
        x2 = torch.cat([xp, xp]) if cfg else xp
        guided_update_(x2, ep, a, ce, cz, w=w if cfg else None, noise=zp, seeds=seeds if mode == "philox" else None, step=step,
                       speech_len=sl)
        for b, n in enumerate(lens):
            assert torch.equal(x2[b, :n], want[b, :n]), f"utterance {b}: valid rows differ from the old chain"
            assert torch.equal(x2[b, n:], torch.zeros_like(x2[b, n:])), f"utterance {b}: padded rows must be exactly 0"
        if cfg:
            assert torch.equal(x2[B:], x2[:B])
        results.append(x2.clone())
    assert torch.equal(results[0], results[1]), "NaN in padded rows of x / eps2 / noise changed a bit"


def test_per_utterance_guidance_is_each_utterances_cfg_combine():
    B, N, d = 3, 130, 256
    x = hash_normal((B, N, d), "x", 1).to(DEV)
    eps2 = hash_normal((2 * B, N, d), "e", 2).to(DEV)
    a, ce, cz = (torch.full((B,), v, device=DEV) for v in (1.05, -0.2, 0.0))
    ws = [5.0, 1.5, 0.0]
    x2 = torch.cat([x, x])
    guided_update_(x2, eps2, a, ce, cz, w=torch.tensor(ws, device=DEV))
    for b, wv in enumerate(ws):
        e2 = torch.cat([eps2[b:b + 1], eps2[B + b:B + b + 1]])
        want = _old_chain(x[b:b + 1], e2, None, a[b:b + 1], ce[b:b + 1], cz[b:b + 1], wv, True)
        assert torch.equal(x2[b:b + 1], want) and torch.equal(x2[B + b:B + b + 1], want)


def test_philox_noise_is_the_padded_layout_index():
    """utterance b's noise on row r is ditto_noise_normal's at (seed, step) whatever the padded length"""
    B, d, step = 2, 256, 5
    seeds = torch.tensor([11, 12], device=DEV)
    a, ce, cz = (torch.full((B,), v, device=DEV) for v in (0.0, 0.0, 1.0))
    outs = []
    for N in (40, 90):
        x2 = torch.zeros(B, N, d, device=DEV)
        guided_update_(x2, torch.zeros_like(x2), a, ce, cz, seeds=seeds, step=step,
                       speech_len=torch.tensor([40, 33], dtype=torch.int32, device=DEV))
        outs.append(x2)
        want = _noise_normal(B, N, d, seeds, step)
        assert torch.equal(x2[0, :40], want[0, :40]) and torch.equal(x2[1, :33], want[1, :33])
    assert torch.equal(outs[0], outs[1][:, :40])
