"""-m gpu: the second-order multistep solver through the model — SpeechGenerator.sample_guided_packed(solver="dpmpp2m") and
guided_stream(solver="dpmpp2m").

(a) the closed call equals, bit for bit, the unfused chain under the same kernel class: engine.forward_packed over [x; x] x [text;
    null], then ditto_multistep_update_packed with the step's coefficients — with and without speech prompts, whose rows come back
    bit-equal;
(b) it agrees with the float64 restatement of the solver (tests/multistep_ref.py) driven by the same forwards, per utterance within
    the loop tolerance of test_gpu_guided_sampler.py (rel-L2 <= 2e-2);
(c) a request stream under a pinned class: every request, served among neighbours of which one is admitted and one retires while it
    is in flight (two regroups move live history), is torch.equal to sample_guided_packed(solver="dpmpp2m") of it alone; a
    steady-state step allocates nothing."""
import ctypes as C

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.sampler import SpeechGenerator, multistep_schedule
from ditto_tts_amd.synth import hash_normal
from gpu_util import rel_l2
from multistep_ref import Solver
from test_gpu_stream_sampler import SMALL, T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = SMALL                    # d = 256, 2 layers, head_dim 64
LENS, TEXTS = (70, 64, 129), (48, 20, 33)
PROMPTS = (30, 0, 100)
GUIDANCE = [3.0, 2.0, 4.5]
N_STEPS = 4
PIN = 4096


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


CU, CT, CN = _cu(LENS), _cu(TEXTS), _cu([T_NULL] * 3)
S, D = CU[-1], CFG.hidden_dim


@pytest.fixture(scope="module")
def sg():
    return SpeechGenerator(ditto_model=_model(CFG, seed=3), device=DEV)


@pytest.fixture(scope="module")
def inputs():
    return (hash_normal((CT[-1], CFG.text_dim), "msl_text", 1).to(DEV), hash_normal((CN[-1], CFG.text_dim), "msl_null", 2).to(DEV),
            hash_normal((S, D), "msl_start", 3).to(DEV))


def _closed(sg, inputs, prompts=None, guidance=GUIDANCE):
    text, null, start = inputs
    kw = dict(guidance=guidance, null_text_emb=null, null_text_cu_seqlens=CN) if guidance is not None else {}
    return sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, cond_by_audio=True, solver="dpmpp2m", prompt_lengths=prompts,
                                   **kw)


def _forward2(eng, inputs, x, t_val, guided):
    """the step's forward, unfused: eps over [x; x] x [text; null] (or over x x text)"""
    text, null, _ = inputs
    if not guided:
        cond = eng.prepare_text_packed(text, CT)
        return eng.forward_packed(x, cond, torch.full((3,), t_val, device=DEV), CU, max_seqlen=max(LENS))
    cond = eng.prepare_text_packed(torch.cat([text, null]).contiguous(), CT + [CT[-1] + c for c in CN[1:]])
    return eng.forward_packed(x, cond, torch.full((6,), t_val, device=DEV), CU + [S + c for c in CU[1:]], max_seqlen=max(LENS))


@pytest.mark.parametrize("guided", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("prompts", [None, PROMPTS], ids=["noprompts", "prompts"])
@torch.no_grad()
def test_closed_call_is_the_unfused_chain_bit_for_bit(sg, inputs, prompts, guided):
    lib, eng = hip.lib(), sg.ditto_model.engine(torch.device("cuda:0"))
    halves = 2 if guided else 1
    with hip.batch_class(PIN):
        got = _closed(sg, inputs, prompts, GUIDANCE if guided else None)
        x2 = torch.cat([inputs[2]] * halves).contiguous()
        q = torch.full((S, D), float("nan"), device=DEV)               # the first step must not read it
        w = torch.tensor(GUIDANCE, device=DEV) if guided else None
        cud = torch.tensor(CU, dtype=torch.int32, device=DEV)
        pl = None if prompts is None else torch.tensor(prompts, dtype=torch.int32, device=DEV)
        for t_val, a, kx, ke, b, g, use_prev in multistep_schedule(sg.alphas_cumprod, N_STEPS):
            eps2 = _forward2(eng, inputs, x2, t_val, guided)
            hip.check(lib.ditto_multistep_update_packed(x2.data_ptr(), eps2.data_ptr(), q.data_ptr(),
                                                        C.byref(hip.MultistepCoef(a, kx, ke, b, g, 0.0, int(use_prev), 0)), None,
                                                        None if w is None else w.data_ptr(), cud.data_ptr(),
                                                        None if pl is None else pl.data_ptr(), 3, S, max(LENS), D, int(guided),
                                                        torch.cuda.current_stream().cuda_stream))
    assert got.shape == (S, D) and torch.isfinite(got).all()
    assert torch.equal(got, x2[:S]), f"rel-L2 {rel_l2(got.cpu(), x2[:S].cpu()):.3e} against the unfused chain"
    if prompts is not None:
        for b, p in enumerate(prompts):
            assert torch.equal(got[CU[b]:CU[b] + p], inputs[2][CU[b]:CU[b] + p]), "the prompt rows must come back bit-equal"
            assert not torch.equal(got[CU[b] + p:CU[b + 1]], inputs[2][CU[b] + p:CU[b + 1]])


@torch.no_grad()
def test_closed_call_against_the_float64_restatement_on_the_same_forwards(sg, inputs):
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    with hip.batch_class(PIN):
        got = _closed(sg, inputs)
        ref = Solver(sg.alphas_cumprod.cpu(), N_STEPS)
        y = inputs[2].double()
        wrow = torch.cat([torch.full((n, 1), GUIDANCE[b], dtype=torch.float64) for b, n in enumerate(LENS)]).to(DEV)
        for i, t_val in enumerate(ref.taus):
            yf = y.float()
            eps2 = _forward2(eng, inputs, torch.cat([yf, yf]).contiguous(), t_val, True).double()
            c, u = eps2[:S], eps2[S:]
            y = ref.step(i, y, u + wrow * (c - u))
    for b in range(3):
        r = rel_l2(got[CU[b]:CU[b + 1]].cpu(), y[CU[b]:CU[b + 1]].cpu())
        print(f"utterance {b}: rel-L2 {r:.3e} against the float64 restatement")
        assert r <= 2e-2, f"utterance {b}: rel-L2 {r:.3e}"


# ---------------------------------------------------------------------------------------------------------------- the stream
# requests: (generated frames, prompt rows, text rows, n_steps).  Request 1 retires after step 2, request 2 is admitted at step 2:
# both regroups (steps 2 and 3) move the live history of request 0, the second one also request 2's, behind its prompt
REQ = [(70, 0, 48, 4), (64, 0, 20, 2), (99, 30, 33, 3)]
ARRIVALS = {0: [0, 1], 1: [2]}
CAPS = dict(max_rows=330, max_utterances=3, max_text_rows=256)


def _req_data():
    prompts = [hash_normal((p, D), "mss_prompt", k) if p else None for k, (_, p, _, _) in enumerate(REQ)]
    texts = [hash_normal((t, CFG.text_dim), "mss_text", k) for k, (_, _, t, _) in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, CFG.text_dim), "mss_null", k) for k in range(len(REQ))]
    return prompts, texts, nulls


def _solo(sg, k, data):
    prompts, texts, nulls = data
    g, p, t, steps = REQ[k]
    audio = torch.zeros(p + g, D)
    if p:
        audio[:p] = prompts[k]
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=steps, guidance=2.0 + k,
                                  null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([700 + k]),
                                  prompt_lengths=[p] if p else None, solver="dpmpp2m")
    return out[p:]


@torch.no_grad()
def test_stream_requests_equal_their_solo_runs_bit_for_bit(sg):
    data = _req_data()
    prompts, texts, nulls = data
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, solver="dpmpp2m", **CAPS)
        results, handles, step, members = {}, {}, 0, []
        while step == 0 or stream.pending or stream.active:
            for k in ARRIVALS.get(step, []):
                g, p, t, steps = REQ[k]
                h = stream.submit(texts[k], g, seed=700 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps, prompt=prompts[k])
                handles[h.id] = k
            done = stream.step()
            members.append(stream.batch.B)
            for h, out in done:
                results[handles[h.id]] = out.clone()
            step += 1
        assert step == 4 and members == [2, 3, 2, 2] and sorted(results) == [0, 1, 2]
        for k in range(3):
            solo = _solo(sg, k, data)
            assert results[k].shape == (REQ[k][0], D) and torch.isfinite(solo).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"
        # the solver matters: the same request through the DDIM stream gives other latents
        ddim = sg.guided_stream(guided=True, **CAPS)
        ddim.submit(texts[0], REQ[0][0], seed=700, guidance=2.0, null_text_emb=nulls[0], n_steps=4)
        (_, other), = ddim.drain()
        assert not torch.equal(other, results[0])


@torch.no_grad()
def test_steady_state_step_allocates_nothing(sg):
    prompts, texts, nulls = _req_data()
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, solver="dpmpp2m", **CAPS)
        stream.submit(texts[2], 99, seed=702, guidance=2.0, null_text_emb=nulls[2], n_steps=8, prompt=prompts[2])
        assert stream.step() == [] and stream.step() == []
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(4):
            assert stream.step() == []
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        (h, out), = stream.drain()
    assert out.shape == (99, D) and torch.isfinite(out).all()
