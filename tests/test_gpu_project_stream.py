"""-m gpu: projected guidance (APG) through the model in a request stream — guided_stream(project=True),
submit(guidance_projection=, guidance_norm_threshold=, guidance_momentum=).

The model, CFG, PIN, capacities, lengths, arrivals and seeds are tests/test_gpu_refresh_stream.py's.  Four requests under a pinned
batch_class: 0 without an interval, projected with eta = 0, beta = -0.5 and a threshold r; 1 with a speech prompt, eta = 0.5; 2 with the
guidance interval (10, 35), eta = 0; 3 without any projection argument.  They arrive and leave at different steps, so the stream runs
steps of kinds {3, 3}, {3, 3, 0}, {3, 3, 3}, one step [3, 0, 1] with all three kinds — request 1's last step, request 2's last step and
request 3's first — and steps in which only request 3 is in flight, which run the entry they run in a stream without project=True.
The recorded trace (members, G, entry) is asserted.  Each result is torch.equal to sample_guided_packed(guidance_projection=, ...) of
that request alone; the parameters matter; a project stream nobody asks anything of is the plain stream bit for bit; steady-state
steps with projected requests in flight allocate nothing; a prediction="v" stream serves the arguments the same way.  What projected
guidance does to speech quality is not measured here.

How r was picked: the threshold acts when the RMS of the x0-space direction ke (c - u) over the window is above r.  c and u are two
forwards of one model on different conditioning (a text against the null text), fp32 numbers of the order of the state itself, so
their difference scaled by |ke| = sigma / alpha >= 0.1 at every timestep above 0 stands orders of magnitude above R_THRESHOLD = 1e-3
unless the two forwards agree to three digits — and the test asserts that the threshold changes the result, so it fails if they did."""
import pytest
import torch

from ditto_tts_amd import hip
from gpu_util import rel_l2
from test_gpu_refresh_stream import ARRIVALS, CAPS, CFG, D, DEV, PIN, REQ, _model
from test_gpu_stream_sampler import T_NULL
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.synth import hash_normal

pytestmark = pytest.mark.gpu
R_THRESHOLD = 1e-3
# request -> its projection arguments (None: it passes none)
PROJ = [dict(guidance_projection=0.0, guidance_norm_threshold=R_THRESHOLD, guidance_momentum=-0.5), dict(guidance_projection=0.5),
        dict(guidance_projection=0.0), None]
MIXED, TAGS = "ditto_guided_step_packed_project_mixed_opts", "ditto_guided_step_packed_tags_opts"
# (who is in flight, how many of them are guided, the entry) per stream step; kinds: {3, 3} | {3, 3, 0} x 2 | {3, 3, 3} x 3 | [3, 0, 1] |
# request 3 alone, three times
TRACE = [([0, 1], 2, MIXED), ([0, 1, 2], 2, MIXED), ([0, 1, 2], 2, MIXED), ([0, 1, 2], 3, MIXED), ([0, 1, 2], 3, MIXED),
         ([0, 1, 2], 3, MIXED), ([1, 2, 3], 2, MIXED), ([3], 1, TAGS), ([3], 1, TAGS), ([3], 1, TAGS)]
KINDS = [[3, 3], [3, 3, 0], [3, 3, 0], [3, 3, 3], [3, 3, 3], [3, 3, 3], [3, 0, 1], [1], [1], [1]]


@pytest.fixture(scope="module")
def sg():
    return SpeechGenerator(ditto_model=_model(CFG, seed=3), device=DEV)


@pytest.fixture(scope="module")
def data():
    prompts = [hash_normal((p, D), "rfs_prompt", k) if p else None for k, (_, p, _, _, _, _) in enumerate(REQ)]
    texts = [hash_normal((t, CFG.text_dim), "rfs_text", k) for k, (_, _, t, _, _, _) in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, CFG.text_dim), "rfs_null", k) for k in range(len(REQ))]
    return prompts, texts, nulls


def _solo(sg, k, data, proj, prediction="eps", steps=None, interval="own"):
    prompts, texts, nulls = data
    g, p, t, n_steps, own, _ = REQ[k]
    audio = torch.zeros(p + g, D)
    if p:
        audio[:p] = prompts[k]
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=steps or n_steps, eta=1.0, guidance=2.0 + k,
                                  null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([700 + k]),
                                  prompt_lengths=[p] if p else None, guidance_interval=own if interval == "own" else interval,
                                  prediction=prediction, **(proj or {}))
    return out[p:]


def _run(sg, data, project_stream, with_args, trace=None, kinds=None):
    """the four requests through one stream; `with_args` False: nobody passes a projection argument"""
    prompts, texts, nulls = data
    stream = sg.guided_stream(guided=True, **CAPS, **({"project": True} if project_stream else {}))
    results, handles, step = {}, {}, 0
    if trace is not None:
        run, call = stream.batch.step, hip.call

        def recorded(a):
            names = []

            def logged(name, **kw):
                names.append(name)
                return call(name, **kw)

            hip.call = logged
            try:
                run(a)
            finally:
                hip.call = call
            entry, = [n for n in names if n.startswith("ditto_guided_step_packed")]
            trace.append(([handles[h.id] for h in a.handles], a.G, entry))
            kinds.append(list(a.kind))

        stream.batch.step = recorded
    while step == 0 or stream.pending or stream.active:
        for k in ARRIVALS.get(step, []):
            g, p, t, steps, interval, _ = REQ[k]
            h = stream.submit(texts[k], g, seed=700 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps, eta=1.0,
                              prompt=prompts[k], guidance_interval=interval, **((PROJ[k] or {}) if with_args else {}))
            handles[h.id] = k
        for h, out in stream.step():
            results[handles[h.id]] = out.clone()
        step += 1
    return results, step


@torch.no_grad()
def test_stream_requests_with_projected_guidance_equal_their_solo_runs_bit_for_bit(sg, data):
    with hip.batch_class(PIN):
        trace, kinds = [], []
        results, steps = _run(sg, data, True, True, trace, kinds)
        assert steps == len(TRACE) and sorted(results) == [0, 1, 2, 3]
        assert trace == TRACE and kinds == KINDS
        for k in range(4):
            solo = _solo(sg, k, data, PROJ[k])
            assert results[k].shape == (REQ[k][0], D) and torch.isfinite(solo).all() and torch.isfinite(results[k]).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"
        # request 3 passes nothing: its result is the one of a stream made without project=True
        plain, _ = _run(sg, data, False, False)
        assert torch.equal(results[3], plain[3])
        # the parameters matter: request 0 without the projection, and without the threshold alone
        none = _solo(sg, 0, data, None)
        no_r = _solo(sg, 0, data, {k: v for k, v in PROJ[0].items() if k != "guidance_norm_threshold"})
        print(f"request 0: rel-L2 to the call without projection {rel_l2(results[0].cpu(), none.cpu()):.3e}, without the threshold "
              f"{rel_l2(results[0].cpu(), no_r.cpu()):.3e}")
        assert torch.isfinite(none).all() and torch.isfinite(no_r).all()
        assert not torch.equal(results[0], none) and not torch.equal(results[0], no_r) and not torch.equal(none, no_r)
        assert torch.equal(none, plain[0])


@torch.no_grad()
def test_a_project_stream_nobody_asks_anything_of_is_the_plain_stream_bit_for_bit(sg, data):
    with hip.batch_class(PIN):
        trace, kinds = [], []
        got, steps = _run(sg, data, True, False, trace, kinds)
        want, steps_plain = _run(sg, data, False, False)
        assert steps == steps_plain and sorted(got) == sorted(want) == [0, 1, 2, 3]
        assert MIXED not in [e for _, _, e in trace] and 3 not in sum(kinds, [])
        for k in range(4):
            assert torch.isfinite(want[k]).all() and torch.equal(got[k], want[k]), k
        plain = sg.guided_stream(guided=True, **CAPS)
        with pytest.raises(ValueError, match="project=True"):
            plain.submit(data[1][0], 70, seed=700, guidance=2.0, null_text_emb=data[2][0], n_steps=4, guidance_projection=0.0)
        assert plain.pending == 0


@torch.no_grad()
def test_steps_with_projected_requests_in_flight_allocate_nothing(sg, data):
    prompts, texts, nulls = data
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, project=True, **CAPS)
        stream.submit(texts[0], 70, seed=700, guidance=2.0, null_text_emb=nulls[0], n_steps=8, eta=1.0, **PROJ[0])
        stream.submit(texts[1], 60, seed=701, guidance=3.0, null_text_emb=nulls[1], n_steps=8, eta=1.0, prompt=prompts[1])
        assert stream.step() == [] and stream.step() == []
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(5):
            assert stream.step() == []
            assert [r.project_kind_now() for r in stream._active] == [hip.KIND_PROJECT, hip.KIND_CFG]
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        outs = stream.drain()
        assert len(outs) == 2 and all(torch.isfinite(o).all() for _, o in outs)


@torch.no_grad()
def test_a_v_prediction_stream_serves_a_prompted_projected_request_equal_to_its_solo_run(sg, data):
    prompts, texts, nulls = data
    proj = dict(guidance_projection=0.25, guidance_norm_threshold=R_THRESHOLD, guidance_momentum=-0.5)
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, project=True, prediction="v", **CAPS)
        stream.submit(texts[1], REQ[1][0], seed=701, guidance=3.0, null_text_emb=nulls[1], n_steps=5, eta=1.0, prompt=prompts[1],
                      guidance_interval=(5, 45), **proj)
        (_, got), = stream.drain()
        solo = _solo(sg, 1, data, proj, prediction="v", steps=5, interval=(5, 45))
        assert torch.isfinite(solo).all() and torch.equal(got, solo), f"rel-L2 {rel_l2(got.cpu(), solo.cpu()):.3e}"
