"""-m gpu: guidance reuse through the model in a request stream — guided_stream(refresh=True), submit(guidance_refresh=k).

Four requests under a pinned batch_class: k = 2, k = 3 with a speech prompt, k = 2 with a guidance interval, and one without the
argument.  They arrive and leave at different steps, so the stream runs steps in which nobody refreshes (G = 0), some do and everyone
does; each result is torch.equal to sample_guided_packed(guidance_refresh=k) of that request alone.  k matters (k = 2 against k = 1),
a refresh stream whose requests never reuse is the plain stream bit for bit, steps with a reusing request in flight allocate
nothing, and a prediction="v" stream serves the argument the same way.  What the approximation does to speech quality is not
measured here."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.synth import hash_normal
from gpu_util import rel_l2
from test_gpu_stream_sampler import T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = DiTTOConfig(256, 2, 4, 256, 256, 50)
D = CFG.hidden_dim
PIN = 4096
# (generated frames, prompt rows, text rows, n_steps, interval, k).  Step kinds at their own step index (F refresh, U reuse, P plain):
#   0: F U F U F U      1: F U U F U U F      2: P P F U F P (timesteps 49, 41, 32, 24, 16, 7)      3: F F F F
REQ = [(70, 0, 48, 6, None, 2), (60, 30, 20, 7, None, 3), (80, 0, 33, 6, (10, 35), 2), (40, 0, 7, 4, None, None)]
ARRIVALS = {0: [0, 1], 1: [2], 3: [3]}                  # submitted AFTER this many steps; 3 waits for a free slot
CAPS = dict(max_rows=256, max_utterances=3, max_text_rows=256)
# (who is in flight, how many of them refresh) per stream step: G = B, G = 0 and 0 < G < B all occur
TRACE = [([0, 1], 2), ([0, 1, 2], 0), ([0, 1, 2], 1), ([0, 1, 2], 2), ([0, 1, 2], 1), ([0, 1, 2], 1), ([1, 2, 3], 2), ([3], 1), ([3], 1),
         ([3], 1)]


@pytest.fixture(scope="module")
def sg():
    return SpeechGenerator(ditto_model=_model(CFG, seed=3), device=DEV)


@pytest.fixture(scope="module")
def data():
    prompts = [hash_normal((p, D), "rfs_prompt", k) if p else None for k, (_, p, _, _, _, _) in enumerate(REQ)]
    texts = [hash_normal((t, CFG.text_dim), "rfs_text", k) for k, (_, _, t, _, _, _) in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, CFG.text_dim), "rfs_null", k) for k in range(len(REQ))]
    return prompts, texts, nulls


def _solo(sg, k, data, refresh):
    prompts, texts, nulls = data
    g, p, t, steps, interval, _ = REQ[k]
    audio = torch.zeros(p + g, D)
    if p:
        audio[:p] = prompts[k]
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=steps, eta=1.0, guidance=2.0 + k,
                                  null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([700 + k]),
                                  prompt_lengths=[p] if p else None, guidance_interval=interval, guidance_refresh=refresh)
    return out[p:]


def _run(sg, data, refresh_stream, with_k, trace=None):
    """the four requests through one stream; `with_k` False: nobody passes guidance_refresh"""
    prompts, texts, nulls = data
    stream = sg.guided_stream(guided=True, **CAPS, **({"refresh": True} if refresh_stream else {}))
    results, handles, step = {}, {}, 0
    if trace is not None:
        run = stream.batch.step

        def recorded(a):
            trace.append(([handles[h.id] for h in a.handles], a.G))
            run(a)

        stream.batch.step = recorded
    while step == 0 or stream.pending or stream.active:
        for k in ARRIVALS.get(step, []):
            g, p, t, steps, interval, kk = REQ[k]
            kw = dict(guidance_refresh=kk) if with_k else {}
            h = stream.submit(texts[k], g, seed=700 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps, eta=1.0,
                              prompt=prompts[k], guidance_interval=interval, **kw)
            handles[h.id] = k
        for h, out in stream.step():
            results[handles[h.id]] = out.clone()
        step += 1
    return results, step


@torch.no_grad()
def test_stream_requests_with_guidance_refresh_equal_their_solo_runs_bit_for_bit(sg, data):
    prompts, texts, nulls = data
    with hip.batch_class(PIN):
        trace = []
        results, steps = _run(sg, data, True, True, trace)
        assert steps == len(TRACE) and sorted(results) == [0, 1, 2, 3]
        assert trace == TRACE
        for k in range(4):
            solo = _solo(sg, k, data, REQ[k][5])
            assert results[k].shape == (REQ[k][0], D) and torch.isfinite(solo).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"
        # k matters: request 0 with k = 1 (every guided step refreshes) gives other latents, those of the call without the argument
        one = sg.guided_stream(guided=True, refresh=True, **CAPS)
        one.submit(texts[0], REQ[0][0], seed=700, guidance=2.0, null_text_emb=nulls[0], n_steps=REQ[0][3], eta=1.0, guidance_refresh=1)
        (_, other), = one.drain()
        assert not torch.equal(other, results[0])
        assert torch.equal(other, _solo(sg, 0, data, None))


@torch.no_grad()
def test_a_refresh_stream_whose_requests_never_reuse_is_the_plain_stream_bit_for_bit(sg, data):
    with hip.batch_class(PIN):
        got, steps = _run(sg, data, True, False)
        want, steps_plain = _run(sg, data, False, False)
        assert steps == steps_plain and sorted(got) == sorted(want) == [0, 1, 2, 3]
        for k in range(4):
            assert torch.isfinite(want[k]).all() and torch.equal(got[k], want[k]), k
        plain = sg.guided_stream(guided=True, **CAPS)
        with pytest.raises(ValueError, match="refresh=True"):
            plain.submit(data[1][0], 70, seed=700, guidance=2.0, null_text_emb=data[2][0], n_steps=4, guidance_refresh=2)
        assert plain.pending == 0


@torch.no_grad()
def test_steps_with_a_reusing_request_in_flight_allocate_nothing(sg, data):
    prompts, texts, nulls = data
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, refresh=True, **CAPS)
        stream.submit(texts[0], 70, seed=700, guidance=2.0, null_text_emb=nulls[0], n_steps=8, eta=1.0, guidance_refresh=3)
        stream.submit(texts[1], 60, seed=701, guidance=3.0, null_text_emb=nulls[1], n_steps=8, eta=1.0, prompt=prompts[1],
                      guidance_refresh=4)
        assert stream.step() == [] and stream.step() == []           # kinds F F, U U
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        kinds = []
        for _ in range(5):                                            # U U (no regroup), F U, U F, U U, F U
            assert stream.step() == []
            kinds.append([r.kinds[r.i - 1] for r in stream._active])
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        U, F = hip.KIND_REUSE, hip.KIND_REFRESH
        assert kinds == [[U, U], [F, U], [U, F], [U, U], [F, U]]
        outs = stream.drain()
        assert len(outs) == 2 and all(torch.isfinite(o).all() for _, o in outs)


@torch.no_grad()
def test_a_v_prediction_stream_request_with_guidance_refresh_equals_its_solo_run(sg, data):
    prompts, texts, nulls = data
    g, p, t = 60, 30, 20                                               # request 1's rows: a prompt in front
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, refresh=True, prediction="v", **CAPS)
        stream.submit(texts[1], g, seed=701, guidance=3.0, null_text_emb=nulls[1], n_steps=5, eta=1.0, prompt=prompts[1],
                      guidance_interval=(5, 45), guidance_refresh=2)
        (_, got), = stream.drain()
        audio = torch.zeros(p + g, D)
        audio[:p] = prompts[1]
        solo = sg.sample_guided_packed(texts[1].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=5, eta=1.0, guidance=3.0,
                                       null_text_emb=nulls[1].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([701]),
                                       prompt_lengths=[p], guidance_interval=(5, 45), guidance_refresh=2, prediction="v")[p:]
        assert torch.isfinite(solo).all() and torch.equal(got, solo), f"rel-L2 {rel_l2(got.cpu(), solo.cpu()):.3e}"
