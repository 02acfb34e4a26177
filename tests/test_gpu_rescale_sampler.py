"""-m gpu: guidance rescale through the model — SpeechGenerator.sample_guided_packed(guidance_rescale=) and
GuidedStream.submit(guidance_rescale=).

No model-level tolerance: the formula is held to its fp64 reference at kernel level (test_gpu_rescale_kernel.py); here everything is
COMPOSITION and torch.equal.  Closed call, both solvers, under a pinned kernel class: guidance_rescale = 0.0 is the call without the
argument; a call with it is a chain composed here — the packed forward over [x; x], ditto_guidance_rescale_packed on its eps, then
the EXISTING update entry with coef_out in the place of ce (ke) — with seeds and eta = 1 for ddim, with prompts (whose rows come back
bit-equal), and with a guidance interval, whose outside steps are the existing unguided entry; in a batch with phi = [0.7, 0, 0.3] the
phi = 0 utterance has the bits of the call without the argument.  Stream, ddim and 2M: requests with different phi, guidance, prompts
and (ddim) intervals, arriving and leaving, each torch.equal to its solo closed call; a steady-state rescaled step allocates nothing."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator, guided_steps, multistep_schedule, strided_schedule
from ditto_tts_amd.synth import hash_normal
from gpu_util import rel_l2, stream as _s
from test_gpu_stream_sampler import T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = DiTTOConfig(256, 2, 4, 256, 256, 50)
LENS, TEXTS = (96, 50, 7), (40, 12, 5)
PROMPTS = (20, 0, 6)                              # the last: P_b = n_b - 1
GUIDANCE = [5.0, 2.0, 3.5]
PHI = [0.7, 0.0, 0.3]
SEEDS = [21, 22, 23]
N_STEPS = 4                                       # timesteps 49, 36, 24, 12
MIDDLE = (20, 40)
B = 3
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
    return (hash_normal((CT[-1], CFG.text_dim), "rs_text", 1).to(DEV), hash_normal((CN[-1], CFG.text_dim), "rs_null", 2).to(DEV),
            hash_normal((S, D), "rs_start", 3).to(DEV))


def _closed(sg, inputs, solver, prompts=None, **kw):
    text, null, start = inputs
    return sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, eta=1.0 if solver == "ddim" else 0.0, seeds=torch.tensor(SEEDS),
                                   cond_by_audio=True, batch_class=B, prompt_lengths=prompts, solver=solver, guidance=GUIDANCE,
                                   null_text_emb=null, null_text_cu_seqlens=CN, **kw)


@pytest.fixture(scope="module")
def today(sg, inputs):
    """the calls without the argument, computed once: solver -> latents"""
    with torch.no_grad():
        return {solver: _closed(sg, inputs, solver) for solver in ("ddim", "dpmpp2m")}


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_phi_zero_is_the_call_without_the_argument(sg, inputs, today, solver):
    assert torch.isfinite(today[solver]).all()
    assert torch.equal(_closed(sg, inputs, solver, guidance_rescale=0.0), today[solver])
    assert torch.equal(_closed(sg, inputs, solver, guidance_rescale=None), today[solver])
    # per utterance: phi = [0.7, 0, 0.3] leaves the phi = 0 utterance's bits alone and moves the others
    got = _closed(sg, inputs, solver, guidance_rescale=PHI)
    assert torch.isfinite(got).all()
    for b in range(B):
        same = torch.equal(got[CU[b]:CU[b + 1]], today[solver][CU[b]:CU[b + 1]])
        assert same == (PHI[b] == 0.0), (b, same)


def _chain(sg, inputs, solver, prompts, interval, phi):
    """the closed call composed from the forward, the statistics entry and the EXISTING update entries"""
    text, null, start = inputs
    lib = hip.lib()
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    multistep = solver == "dpmpp2m"
    sched = multistep_schedule(sg.alphas_cumprod, N_STEPS) if multistep else strided_schedule(sg.alphas_cumprod, N_STEPS, 1.0)
    mask = guided_steps(sched, interval)
    cond2 = eng.prepare_text_packed(torch.cat([text, null]).contiguous(), CT + [CT[-1] + c for c in CN[1:]])
    cond1 = eng.prepare_text_packed(text, CT)
    off2, off1 = eng.guided_offsets_packed(CU, S, N, True), eng.guided_offsets_packed(CU, S, N, False)
    opts2, opts1 = hip.CallOpts(class_rows=2 * B * N), hip.CallOpts(class_rows=B * N)
    cu2 = CU + [S + c for c in CU[1:]]
    x2 = torch.cat([start, torch.full_like(start, float("nan"))]).contiguous()
    w = torch.tensor(GUIDANCE, device=DEV)
    phid = torch.tensor(phi, dtype=torch.float32, device=DEV)
    seeds = torch.tensor(SEEDS, device=DEV)
    q = torch.full((S, D), float("nan"), device=DEV)
    pl = None if prompts is None else torch.tensor(prompts, dtype=torch.int32, device=DEV)
    kw = {} if pl is None else dict(prompt_len=pl)
    ptr = lambda t: None if t is None else t.data_ptr()
    scales, stale = [], True
    for i, row in enumerate(sched):
        if not mask[i]:                                   # outside the interval: the existing unguided entry on the conditional half
            stale = True
            t = torch.full((B,), row[0], device=DEV)
            if multistep:
                eng.guided_step_packed_multistep_(x2[:S], cond1, t, B, q, hip.MultistepCoef(*row[1:6], 0.0, int(row[6]), 0), offsets=off1,
                                                  opts=opts1, **kw)
            else:
                a, ce, cz = (torch.full((B,), v, device=DEV) for v in row[1:])
                eng.guided_step_packed_(x2[:S], cond1, t, B, a, ce, cz, seeds=seeds if row[3] != 0.0 else None, step=row[0],
                                        offsets=off1, opts=opts1, **kw)
            continue
        if stale:
            x2[S:].copy_(x2[:S])
            stale = False
        eps = eng.forward_packed(x2, cond2, torch.full((2 * B,), row[0], device=DEV), cu2, max_seqlen=N, opts=opts2)
        if multistep:
            coefs = torch.zeros(B, 8, device=DEV)
            coefs[:, :5] = torch.tensor(row[1:6], dtype=torch.float32, device=DEV)
            coefs[:, 5] = w
            coefs.view(torch.int32)[:, 6] = int(row[6])
            out, scale = eng.guidance_rescale_packed(eps, off2[0], phid, B, S, N, coefs=coefs, prompt_len=pl)
            hip.check(lib.ditto_multistep_update_packed(x2.data_ptr(), eps.data_ptr(), q.data_ptr(), None, out.data_ptr(), None,
                                                        off2[0].data_ptr(), ptr(pl), B, S, N, D, 1, _s()))
        else:
            a, ce, cz = (torch.full((B,), v, device=DEV) for v in row[1:])
            sd = seeds if row[3] != 0.0 else None
            out, scale = eng.guidance_rescale_packed(eps, off2[0], phid, B, S, N, w=w, coef_in=ce, prompt_len=pl)
            if pl is None:
                hip.check(lib.ditto_guided_update_packed(x2.data_ptr(), eps.data_ptr(), None, ptr(sd), row[0], w.data_ptr(), a.data_ptr(),
                                                         out.data_ptr(), cz.data_ptr(), off2[0].data_ptr(), B, S, N, D, 1, _s()))
            else:
                hip.check(lib.ditto_guided_update_packed_prompt(x2.data_ptr(), eps.data_ptr(), None, ptr(sd), row[0], w.data_ptr(),
                                                                a.data_ptr(), out.data_ptr(), cz.data_ptr(), off2[0].data_ptr(),
                                                                pl.data_ptr(), B, S, N, D, 1, _s()))
        scales.append(scale.clone())
    return x2[:S].clone(), mask, scales


CHAINS = [("ddim", None, None), ("dpmpp2m", None, None), ("ddim", PROMPTS, None), ("dpmpp2m", PROMPTS, None), ("ddim", None, MIDDLE),
          ("dpmpp2m", PROMPTS, MIDDLE)]


@pytest.mark.parametrize("solver,prompts,interval", CHAINS, ids=[f"{s}-{'prompts' if p else 'noprompts'}-{'interval' if i else 'every'}"
                                                               for s, p, i in CHAINS])
@torch.no_grad()
def test_closed_call_is_the_chain_of_forward_statistics_and_the_existing_update(sg, inputs, solver, prompts, interval):
    start = inputs[2]
    got = _closed(sg, inputs, solver, prompts, guidance_rescale=PHI, guidance_interval=interval)
    want, mask, scales = _chain(sg, inputs, solver, prompts, interval, PHI)
    assert mask == ([True] * 4 if interval is None else [False, True, True, False])
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), f"rel-L2 {rel_l2(got.cpu(), want.cpu()):.3e} against the chain"
    for sc in scales:                                     # the rescale did something, and nothing to the phi = 0 utterance
        assert torch.isfinite(sc).all() and float(sc[1]) == 1.0 and float(sc[0]) != 1.0 and float(sc[2]) != 1.0, sc.tolist()
    plain = _closed(sg, inputs, solver, prompts, guidance_interval=interval)
    assert not torch.equal(got, plain)
    if prompts is not None:
        for b, p in enumerate(prompts):
            assert torch.equal(got[CU[b]:CU[b] + p], start[CU[b]:CU[b] + p]), "the prompt rows must come back bit-equal"


# ---------------------------------------------------------------------------------------------------------------- the stream
# requests: (generated frames, prompt rows, text rows, n_steps, interval (ddim streams only), phi)
REQ = [(70, 0, 40, 4, (20, 40), 0.7), (64, 0, 12, 3, None, None), (50, 30, 33, 4, None, 0.3), (40, 0, 7, 3, (40, 49), 1.0)]
ARRIVALS = {0: [0, 1], 1: [2], 3: [3]}
CAPS = dict(max_rows=260, max_utterances=3, max_text_rows=256)


def _req_data():
    prompts = [hash_normal((r[1], D), "rss_prompt", k) if r[1] else None for k, r in enumerate(REQ)]
    texts = [hash_normal((r[2], CFG.text_dim), "rss_text", k) for k, r in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, CFG.text_dim), "rss_null", k) for k in range(len(REQ))]
    return prompts, texts, nulls


def _solo(sg, k, data, solver):
    prompts, texts, nulls = data
    g, p, t, steps, interval, phi = REQ[k]
    audio = torch.zeros(p + g, D)
    if p:
        audio[:p] = prompts[k]
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=steps, eta=1.0 if solver == "ddim" else 0.0,
                                  guidance=2.0 + k, null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL],
                                  seeds=torch.tensor([900 + k]), prompt_lengths=[p] if p else None, solver=solver,
                                  guidance_interval=interval if solver == "ddim" else None, guidance_rescale=phi)
    return out[p:]


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_stream_requests_equal_their_solo_closed_calls_bit_for_bit(sg, solver):
    data = _req_data()
    prompts, texts, nulls = data
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, solver=solver, **CAPS)
        results, handles, step, kinds = {}, {}, 0, set()
        run = stream.batch.step

        def recorded(a):               # which step kinds occur: (somebody rescaled, guided utterances against utterances in flight)
            kinds.add((any(p > 0 and g for p, g in zip(a.phi, a.in_g)), "all" if a.G == a.B else "none" if a.G == 0 else "some"))
            run(a)

        stream.batch.step = recorded
        while step == 0 or stream.pending or stream.active:
            for k in ARRIVALS.get(step, []):
                g, p, t, steps, interval, phi = REQ[k]
                h = stream.submit(texts[k], g, seed=900 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps,
                                  eta=1.0 if solver == "ddim" else 0.0, prompt=prompts[k],
                                  guidance_interval=interval if solver == "ddim" else None, guidance_rescale=phi)
                handles[h.id] = k
            for h, out in stream.step():
                results[handles[h.id]] = out.clone()
            step += 1
        assert sorted(results) == [0, 1, 2, 3]
        assert (True, "all") in kinds and (solver != "ddim" or (True, "some") in kinds), kinds
        for k in range(4):
            solo = _solo(sg, k, data, solver)
            assert results[k].shape == (REQ[k][0], D) and torch.isfinite(solo).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"
        # the rescale matters: request 0 without it gives other latents
        plain = sg.guided_stream(guided=True, solver=solver, **CAPS)
        plain.submit(texts[0], REQ[0][0], seed=900, guidance=2.0, null_text_emb=nulls[0], n_steps=4, eta=1.0 if solver == "ddim" else 0.0,
                     guidance_interval=REQ[0][4] if solver == "ddim" else None)
        (_, other), = plain.drain()
        assert not torch.equal(other, results[0])


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_steady_state_rescaled_step_allocates_nothing(sg, solver):
    prompts, texts, nulls = _req_data()
    eta = 1.0 if solver == "ddim" else 0.0
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, solver=solver, **CAPS)
        stream.submit(texts[0], 70, seed=900, guidance=2.0, null_text_emb=nulls[0], n_steps=8, eta=eta, guidance_rescale=0.7)
        stream.submit(texts[2], 50, seed=902, guidance=4.0, null_text_emb=nulls[2], n_steps=8, eta=eta, prompt=prompts[2],
                      guidance_interval=(0, 4) if solver == "ddim" else None)       # ddim: never guided — the mixed layout, rescaled
        assert stream.step() == [] and stream.step() == []
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(4):
            assert stream.step() == []
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        outs = stream.drain()
        assert len(outs) == 2 and all(torch.isfinite(o).all() for _, o in outs)
