"""-m gpu: speech-prompted sampling — SpeechGenerator.sample_guided_packed(prompt_lengths=) and GuidedStream.submit(prompt=).

The reference has no prompting; like the strided loop and the guidance this is pinned by its formulas, restated here: for each
utterance alone, eps = oracle.ditto_forward on [prompt; x_gen] for the text and the null text, e = u + w (c - u), and the DDIM update
with oracle.sample_latents_strided's coefficients on the generated rows only.  Loop tolerance: per-utterance rel-L2 <= 2e-2 (DESIGN
§2).  Under a pinned kernel class an utterance's bits depend on its own rows only, so batch against solo and stream against closed call
are torch.equal."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.synth import hash_normal, synthetic_state_dict
from gpu_util import rel_l2
from oracle import ditto_oracle as O
from test_gpu_stream_sampler import C2L2, SMALL, T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (rows N = P + G, prompt rows P, text rows) per utterance
UTT = [(160, 40, 48), (64, 0, 20), (129, 97, 33)]
UTT_128 = [(200, 40, 48), (128, 0, 20), (257, 97, 33)]      # the bf16-stream class refuses launches of fewer than 128 rows
GUIDANCE = [3.0, 2.0, 4.5]
SEEDS = [101, 202, 303]


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _data(cfg, utt):
    audio = [hash_normal((n, cfg.hidden_dim), "pr_audio", k) for k, (n, _, _) in enumerate(utt)]
    texts = [hash_normal((t, cfg.text_dim), "pr_text", k) for k, (_, _, t) in enumerate(utt)]
    nulls = [hash_normal((T_NULL, cfg.text_dim), "pr_null", k) for k in range(len(utt))]
    return audio, texts, nulls


def _sample(sg, cfg, utt, order, data, prompts=True, **kw):
    """sample_guided_packed over utterances `order` of `utt`; returns {k: its [N_k, d] rows}"""
    audio, texts, nulls = data
    cu = _cu([utt[k][0] for k in order])
    args = dict(guidance=[GUIDANCE[k] for k in order], null_text_emb=torch.cat([nulls[k] for k in order]).to(DEV),
                null_text_cu_seqlens=_cu([T_NULL] * len(order)), eta=1.0, n_steps=4)
    if "noises" not in kw:
        args["seeds"] = torch.tensor([SEEDS[k] for k in order])
    if prompts:
        args["prompt_lengths"] = [utt[k][1] for k in order]
    args.update(kw)
    out = sg.sample_guided_packed(torch.cat([texts[k] for k in order]).to(DEV), _cu([utt[k][2] for k in order]),
                                  torch.cat([audio[k] for k in order]).to(DEV), cu, **args)
    return {k: out[cu[j]:cu[j + 1]] for j, k in enumerate(order)}


@torch.no_grad()
def test_prompted_loop_against_the_fp32_restatement():
    cfg, n_steps, w = SMALL, 4, 3.0
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    data = _data(cfg, UTT)
    audio, texts, nulls = data
    cu = _cu([n for n, _, _ in UTT])
    S, d = cu[-1], cfg.hidden_dim
    noises = [hash_normal((S, d), "pr_z", i) for i in range(n_steps)]
    x_T = hash_normal((S, d), "pr_xT", 0)
    # the library: the generated rows start from x_T through cond_by_audio over [prompt; x_T]
    start = [torch.cat([audio[k][:p], x_T[cu[k] + p:cu[k + 1]]]) for k, (n, p, _) in enumerate(UTT)]
    got = _sample(sg, cfg, UTT, [0, 1, 2], (start, texts, nulls), noises=noises, cond_by_audio=True, guidance=w)
    # the restatement, one utterance at a time
    sd = synthetic_state_dict(cfg, seed=3)
    _, _, ac = O.sampler_tables(cfg.diffusion_steps)
    taus = O.strided_timesteps(cfg.diffusion_steps, n_steps)
    for k, (n, p, _) in enumerate(UTT):
        prompt, x = audio[k][:p], x_T[cu[k] + p:cu[k + 1]].clone()
        for i, t_val in enumerate(taus):
            t = torch.full((1,), t_val, dtype=torch.long)
            full = torch.cat([prompt, x])[None]
            c = O.ditto_forward(sd, cfg.num_layers, cfg.num_heads, full, texts[k][None], t)[0, p:]
            u = O.ditto_forward(sd, cfg.num_layers, cfg.num_heads, full, nulls[k][None], t)[0, p:]
            e = u + w * (c - u)
            a, ce, cz = O.ddim_coefficients(ac, t_val, taus[i + 1] if i + 1 < n_steps else -1, 1.0)
            x = a * x + ce * e + cz * noises[i][cu[k] + p:cu[k + 1]]
        r = rel_l2(got[k][p:].cpu(), x)
        print(f"utterance {k} (P {p}, G {n - p}): rel-L2 {r:.3e} against the fp32 restatement")
        assert r <= 2e-2, f"utterance {k}: rel-L2 {r:.3e}"
        assert torch.equal(got[k][:p].cpu(), prompt), "the prompt rows must come back bit-equal"


@pytest.mark.parametrize("cfg,rows,utt", [(SMALL, 4096, UTT), (C2L2, 17408, UTT_128)], ids=["fp32_stream", "bf16_stream"])
@torch.no_grad()
def test_prompted_utterance_in_a_batch_equals_it_alone_under_the_pin(cfg, rows, utt):
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    data = _data(cfg, utt)
    with hip.batch_class(rows):
        if cfg is C2L2:
            assert hip.stream_is_bf16(cfg, 1, 128)
        solo = {k: _sample(sg, cfg, utt, [k], data)[k] for k in range(3)}
        batch = _sample(sg, cfg, utt, [0, 1, 2], data)
        perm = _sample(sg, cfg, utt, [2, 0, 1], data)
        pair = _sample(sg, cfg, utt, [1, 0], data)            # beside a neighbour without a prompt only
    for k in range(3):
        p = utt[k][1]
        assert torch.isfinite(solo[k]).all()
        assert torch.equal(solo[k][:p].cpu(), data[0][k][:p])
        assert torch.equal(batch[k], solo[k]), f"utterance {k}: rel-L2 {rel_l2(batch[k].cpu(), solo[k].cpu()):.3e} against its solo run"
        assert torch.equal(perm[k], solo[k]), k
    assert torch.equal(pair[0], solo[0]) and torch.equal(pair[1], solo[1])


@torch.no_grad()
def test_the_prompt_matters_and_zero_prompts_are_the_plain_call():
    cfg = SMALL
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    data = _data(cfg, UTT)
    audio, texts, nulls = data
    with hip.batch_class(4096):
        a = _sample(sg, cfg, UTT, [0, 1, 2], data)
        other = [audio[0].clone(), audio[1], audio[2]]
        other[0][:UTT[0][1]] = hash_normal((UTT[0][1], cfg.hidden_dim), "pr_other_speaker", 0)
        b = _sample(sg, cfg, UTT, [0, 1, 2], (other, texts, nulls))
        p = UTT[0][1]
        assert not torch.equal(a[0][p:], b[0][p:])             # another speaker's prompt: other generated rows
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        none = _sample(sg, cfg, UTT, [0, 1, 2], data, prompts=False)
        zero = _sample(sg, cfg, UTT, [0, 1, 2], data, prompt_lengths=[0, 0, 0])
    for k in range(3):
        assert torch.equal(zero[k], none[k]), k
    # a prompted utterance draws what an unprompted one of G rows draws: utterance 1 (P = 0) is the plain call's
    assert torch.equal(a[1], none[1])


# ---------------------------------------------------------------------------------------------------------------- the stream
# requests: (generated frames, prompt rows, text rows, n_steps)
REQ = [(120, 40, 48, 4), (64, 0, 20, 6), (32, 97, 33, 5), (100, 30, 7, 4)]
CAPS = dict(max_rows=330, max_utterances=3, max_text_rows=256)
ARRIVALS = {0: [0, 1], 2: [2], 3: [3]}


def _req_data(cfg):
    prompts = [hash_normal((p, cfg.hidden_dim), "prs_prompt", k) if p else None for k, (_, p, _, _) in enumerate(REQ)]
    texts = [hash_normal((t, cfg.text_dim), "prs_text", k) for k, (_, _, t, _) in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, cfg.text_dim), "prs_null", k) for k in range(len(REQ))]
    return prompts, texts, nulls


def _solo_req(sg, cfg, k, data, x_T=None):
    prompts, texts, nulls = data
    g, p, t, steps = REQ[k]
    audio = torch.zeros(p + g, cfg.hidden_dim)
    if p:
        audio[:p] = prompts[k]
    if x_T is not None:
        audio[p:] = x_T
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=steps, eta=1.0, guidance=2.0 + k,
                                  null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([500 + k]),
                                  prompt_lengths=[p], cond_by_audio=x_T is not None)
    assert torch.equal(out[:p].cpu(), audio[:p])
    return out[p:]


@torch.no_grad()
def test_stream_of_prompted_requests_equals_their_solo_runs():
    cfg = SMALL
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    data = _req_data(cfg)
    prompts, texts, nulls = data
    own = hash_normal((REQ[3][0], cfg.hidden_dim), "prs_xT", 3)            # request 3 brings its own x_T [n_frames, d]
    with hip.batch_class(4096):
        stream = sg.guided_stream(guided=True, **CAPS)
        results, handles, step, rows_seen = {}, {}, 0, []
        while step == 0 or stream.pending or stream.active:
            for k in ARRIVALS.get(step, []):
                g, p, t, steps = REQ[k]
                h = stream.submit(texts[k], g, seed=500 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps, eta=1.0,
                                  prompt=prompts[k], x_T=own if k == 3 else None)
                handles[h.id] = k
            for h, out in stream.step():
                results[handles[h.id]] = out.clone()
            rows_seen.append(stream.batch.S)
            step += 1
        assert sorted(results) == [0, 1, 2, 3]
        # admission counts P + n_frames: requests 0 (160 rows) and 1 (64) leave no room for 2 (129) in 330 until 0 retires after step 4
        assert rows_seen[:4] == [224, 224, 224, 224] and rows_seen[4] == 64 + 129 + 130
        for k in range(4):
            solo = _solo_req(sg, cfg, k, data, x_T=own if k == 3 else None)
            assert results[k].shape == (REQ[k][0], cfg.hidden_dim)
            assert torch.isfinite(solo).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"


@torch.no_grad()
def test_prompted_stream_steady_state_allocates_nothing():
    cfg = SMALL
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    prompts, texts, nulls = _req_data(cfg)
    with hip.batch_class(4096):
        stream = sg.guided_stream(guided=True, **CAPS)
        stream.submit(texts[0], 120, seed=500, guidance=2.0, null_text_emb=nulls[0], n_steps=8, eta=1.0, prompt=prompts[0])
        assert stream.step() == [] and stream.step() == []
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(4):
            assert stream.step() == []
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        (h, out), = stream.drain()
    assert out.shape == (120, cfg.hidden_dim) and torch.isfinite(out).all()
