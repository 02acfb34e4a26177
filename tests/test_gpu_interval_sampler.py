"""-m gpu: guidance in a limited interval through the model — SpeechGenerator.sample_guided_packed(guidance_interval=) and
GuidedStream.submit(guidance_interval=).

Closed call, both solvers, with and without speech prompts, under a pinned batch_class: no interval and an interval over every
timestep are today's call bit for bit; an interval over no timestep is the call without guidance; an interval over the middle steps
is a chain composed here from the engine's existing per-step entries (the CFG entry over [x; x], the non-CFG entry over the
conditional half with the texts' own conditioning).  Stream (DDIM): requests with different intervals, one without, one prompted,
arriving and leaving while the guided set changes — every step kind occurs: mixed, everyone guided, nobody guided — each torch.equal to
sample_guided_packed(guidance_interval=) of that request alone; a steady-state mixed step allocates nothing."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator, guided_steps, multistep_schedule, strided_schedule
from ditto_tts_amd.synth import hash_normal
from gpu_util import rel_l2
from test_gpu_stream_sampler import T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = DiTTOConfig(256, 2, 4, 256, 256, 50)
LENS, TEXTS = (160, 64, 97, 33), (48, 20, 33, 7)
PROMPTS = (30, 0, 50, 5)
GUIDANCE = [3.0, 2.0, 4.5, 1.5]
SEEDS = [11, 12, 13, 14]
N_STEPS = 6                                   # timesteps 49, 41, 32, 24, 16, 7
EVERY, NONE, MIDDLE = (0, 49), (8, 15), (10, 35)
B = 4
PIN = 4096


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


CU, CT, CN = _cu(LENS), _cu(TEXTS), _cu([T_NULL] * B)
S, D, N = CU[-1], CFG.hidden_dim, max(LENS)


@pytest.fixture(scope="module")
def sg():
    return SpeechGenerator(ditto_model=_model(CFG, seed=3), device=DEV)


@pytest.fixture(scope="module")
def inputs():
    return (hash_normal((CT[-1], CFG.text_dim), "iv_text", 1).to(DEV), hash_normal((CN[-1], CFG.text_dim), "iv_null", 2).to(DEV),
            hash_normal((S, D), "iv_start", 3).to(DEV))


def _closed(sg, inputs, solver, prompts, guided=True, **kw):
    text, null, start = inputs
    if guided:
        kw.update(guidance=GUIDANCE, null_text_emb=null, null_text_cu_seqlens=CN)
    return sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, eta=1.0 if solver == "ddim" else 0.0, seeds=torch.tensor(SEEDS),
                                   cond_by_audio=True, batch_class=B, prompt_lengths=prompts, solver=solver, **kw)


@pytest.fixture(scope="module")
def today(sg, inputs):
    """today's calls, computed once: (solver, prompted) -> (the guided call, the unguided call), neither with the new argument"""
    out = {}
    with torch.no_grad():
        for solver in ("ddim", "dpmpp2m"):
            for prompts in (None, PROMPTS):
                out[solver, prompts is not None] = (_closed(sg, inputs, solver, prompts), _closed(sg, inputs, solver, prompts, guided=False))
    return out


def test_the_schedule_has_the_timesteps_the_intervals_are_chosen_for(sg):
    taus = [row[0] for row in strided_schedule(sg.alphas_cumprod, N_STEPS, 1.0)]
    assert taus == [49, 41, 32, 24, 16, 7] == [row[0] for row in multistep_schedule(sg.alphas_cumprod, N_STEPS)]


@pytest.mark.parametrize("prompts", [None, PROMPTS], ids=["noprompts", "prompts"])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_no_interval_and_every_step_are_todays_call_and_no_step_is_the_unguided_call(sg, inputs, today, solver, prompts):
    guided, unguided = today[solver, prompts is not None]
    assert torch.isfinite(guided).all() and not torch.equal(guided, unguided)
    assert torch.equal(_closed(sg, inputs, solver, prompts, guidance_interval=None), guided)
    assert torch.equal(_closed(sg, inputs, solver, prompts, guidance_interval=EVERY), guided)
    got = _closed(sg, inputs, solver, prompts, guidance_interval=NONE)
    assert torch.equal(got, unguided), f"rel-L2 {rel_l2(got.cpu(), unguided.cpu()):.3e} against the call without guidance"


@pytest.mark.parametrize("prompts", [None, PROMPTS], ids=["noprompts", "prompts"])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_middle_interval_is_the_chain_of_the_existing_step_entries(sg, inputs, today, solver, prompts):
    text, null, start = inputs
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    got = _closed(sg, inputs, solver, prompts, guidance_interval=MIDDLE)
    multistep = solver == "dpmpp2m"
    sched = multistep_schedule(sg.alphas_cumprod, N_STEPS) if multistep else strided_schedule(sg.alphas_cumprod, N_STEPS, 1.0)
    mask = guided_steps(sched, MIDDLE)
    assert mask == [False, False, True, True, True, False]
    cond2 = eng.prepare_text_packed(torch.cat([text, null]).contiguous(), CT + [CT[-1] + c for c in CN[1:]])
    cond1 = eng.prepare_text_packed(text, CT)
    off2, off1 = eng.guided_offsets_packed(CU, S, N, True), eng.guided_offsets_packed(CU, S, N, False)
    opts2, opts1 = hip.CallOpts(class_rows=2 * B * N), hip.CallOpts(class_rows=B * N)
    x2 = torch.cat([start, torch.full_like(start, float("nan"))]).contiguous()        # the second half is refreshed before its first use
    w = torch.tensor(GUIDANCE, device=DEV)
    seeds = torch.tensor(SEEDS, device=DEV)
    q = torch.full((S, D), float("nan"), device=DEV)
    kw = {} if prompts is None else dict(prompt_len=torch.tensor(prompts, dtype=torch.int32, device=DEV))
    stale = True
    for i, row in enumerate(sched):
        g = mask[i]
        if g and stale:
            x2[S:].copy_(x2[:S])
            stale = False
        stale |= not g
        x, cond, off, opts = (x2, cond2, off2, opts2) if g else (x2[:S], cond1, off1, opts1)
        t = torch.full((2 * B if g else B,), row[0], device=DEV)
        if multistep:
            eng.guided_step_packed_multistep_(x, cond, t, B, q, hip.MultistepCoef(*row[1:6], 0.0, int(row[6]), 0), w=w if g else None,
                                              offsets=off, opts=opts, **kw)
        else:
            a, ce, cz = (torch.full((B,), v, device=DEV) for v in row[1:])
            eng.guided_step_packed_(x, cond, t, B, a, ce, cz, w=w if g else None, seeds=seeds if row[3] != 0.0 else None, step=row[0],
                                    offsets=off, opts=opts, **kw)
    want = x2[:S]
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), f"rel-L2 {rel_l2(got.cpu(), want.cpu()):.3e} against the chain of existing entries"
    guided, unguided = today[solver, prompts is not None]
    assert not torch.equal(got, guided) and not torch.equal(got, unguided)
    if prompts is not None:
        for b, p in enumerate(prompts):
            assert torch.equal(got[CU[b]:CU[b] + p], start[CU[b]:CU[b] + p]), "the prompt rows must come back bit-equal"


# ---------------------------------------------------------------------------------------------------------------- the stream
# requests: (generated frames, prompt rows, text rows, n_steps, interval).  Guided at their own step index: 0 at 2, 3, 4; 1 always;
# 2 at 2, 3, 4; 3 at 0.  In flight / guided per stream step: {0, 1} / {1}; {0, 1, 2} / {1}; {0, 1, 2} / {0, 1} (the guided set
# changes, the members do not); {0, 2, 3} / everyone; {0, 2, 3} / {0, 2}; {0, 2, 3} / {2}; {3} / nobody.
REQ = [(70, 0, 48, 6, (10, 35)), (64, 0, 20, 3, None), (99, 30, 33, 5, (0, 30)), (40, 0, 7, 4, (45, 49))]
ARRIVALS = {0: [0, 1], 1: [2], 3: [3]}
CAPS = dict(max_rows=330, max_utterances=3, max_text_rows=256)
TRACE = [([0, 1], 1), ([0, 1, 2], 1), ([0, 1, 2], 2), ([0, 2, 3], 3), ([0, 2, 3], 2), ([0, 2, 3], 1), ([3], 0)]


def _req_data():
    prompts = [hash_normal((p, D), "ivs_prompt", k) if p else None for k, (_, p, _, _, _) in enumerate(REQ)]
    texts = [hash_normal((t, CFG.text_dim), "ivs_text", k) for k, (_, _, t, _, _) in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, CFG.text_dim), "ivs_null", k) for k in range(len(REQ))]
    return prompts, texts, nulls


def _solo(sg, k, data):
    prompts, texts, nulls = data
    g, p, t, steps, interval = REQ[k]
    audio = torch.zeros(p + g, D)
    if p:
        audio[:p] = prompts[k]
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=steps, eta=1.0, guidance=2.0 + k,
                                  null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([700 + k]),
                                  prompt_lengths=[p] if p else None, guidance_interval=interval)
    return out[p:]


@torch.no_grad()
def test_stream_requests_with_intervals_equal_their_solo_runs_bit_for_bit(sg):
    data = _req_data()
    prompts, texts, nulls = data
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, **CAPS)
        results, handles, step, trace = {}, {}, 0, []
        run = stream.batch.step

        def recorded(a):               # (who is in flight, how many of them are guided) of every step the stream runs
            trace.append(([handles[h.id] for h in a.handles], a.G))
            run(a)

        stream.batch.step = recorded
        while step == 0 or stream.pending or stream.active:
            for k in ARRIVALS.get(step, []):
                g, p, t, steps, interval = REQ[k]
                h = stream.submit(texts[k], g, seed=700 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps, eta=1.0,
                                  prompt=prompts[k], guidance_interval=interval)
                handles[h.id] = k
            done = stream.step()
            for h, out in done:
                results[handles[h.id]] = out.clone()
            step += 1
        assert step == len(TRACE) and sorted(results) == [0, 1, 2, 3]
        assert trace == TRACE
        for k in range(4):
            solo = _solo(sg, k, data)
            assert results[k].shape == (REQ[k][0], D) and torch.isfinite(solo).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"
        # the interval matters: request 0 without it gives other latents
        plain = sg.guided_stream(guided=True, **CAPS)
        plain.submit(texts[0], REQ[0][0], seed=700, guidance=2.0, null_text_emb=nulls[0], n_steps=6, eta=1.0)
        (_, other), = plain.drain()
        assert not torch.equal(other, results[0])


@torch.no_grad()
def test_steady_state_mixed_step_allocates_nothing_and_the_multistep_stream_refuses(sg):
    prompts, texts, nulls = _req_data()
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, **CAPS)
        stream.submit(texts[0], 70, seed=700, guidance=2.0, null_text_emb=nulls[0], n_steps=8, eta=1.0)
        stream.submit(texts[2], 99, seed=702, guidance=4.0, null_text_emb=nulls[2], n_steps=8, eta=1.0, prompt=prompts[2],
                      guidance_interval=(0, 4))                        # no timestep of its schedule: never guided
        assert stream.step() == [] and stream.step() == []
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(4):
            assert stream.step() == []
            assert [r.in_g for r in stream._active] == [True, False]   # one guided, one not: the mixed step
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        outs = stream.drain()
        assert len(outs) == 2 and all(torch.isfinite(o).all() for _, o in outs)
        two_m = sg.guided_stream(guided=True, solver="dpmpp2m", **CAPS)
        with pytest.raises(NotImplementedError, match="ddim"):
            two_m.submit(texts[0], 70, seed=700, guidance=2.0, null_text_emb=nulls[0], n_steps=4, guidance_interval=(10, 35))
        assert two_m.pending == 0
