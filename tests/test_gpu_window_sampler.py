"""-m gpu: speech infilling through the model — SpeechGenerator.sample_guided_packed(suffix_lengths=) and
guided_stream(infill=True).submit(suffix=).  Composition only, torch.equal, under a pinned kernel class:

(a) the closed call equals the unfused chain — engine.forward_packed over [x; x] x [text; null], then the window update entry
    (ditto_guided_update_packed_window, or ditto_multistep_update_window for solver="dpmpp2m") — and both contexts come back bit-equal
    to audio_emb; with a guidance_interval it equals the chain of cfg 1 / cfg 0 window steps;
(b) suffix_lengths all zero equals the call with prompt_lengths alone, and suffix_lengths=None is the call as it was;
(c) a request stream: a request with prefix and suffix, served among arriving and leaving neighbours (suffixed, prompted and plain),
    is torch.equal to its solo closed call, for both solvers; a steady-state step allocates nothing; an infill stream with no
    suffixed request in flight gives the bits of a plain stream."""
import ctypes as C

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.sampler import SpeechGenerator, guided_steps, multistep_schedule, strided_schedule
from ditto_tts_amd.synth import hash_normal
from gpu_util import rel_l2
from test_gpu_stream_sampler import SMALL, T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = SMALL                    # d = 256, 2 layers, head_dim 64
LENS, TEXTS = (70, 64, 129), (48, 20, 33)
PREFIX, SUFFIX = (30, 0, 100), (15, 20, 28)       # both contexts, a suffix only, G = 1 between two contexts
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


def _s():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def sg():
    return SpeechGenerator(ditto_model=_model(CFG, seed=3), device=DEV)


@pytest.fixture(scope="module")
def inputs():
    return (hash_normal((CT[-1], CFG.text_dim), "wsl_text", 1).to(DEV), hash_normal((CN[-1], CFG.text_dim), "wsl_null", 2).to(DEV),
            hash_normal((S, D), "wsl_start", 3).to(DEV))


def _closed(sg, inputs, solver, prompts=PREFIX, suffixes=SUFFIX, guidance=GUIDANCE, **kw):
    text, null, start = inputs
    if guidance is not None:
        kw.update(guidance=guidance, null_text_emb=null, null_text_cu_seqlens=CN)
    kw.setdefault("cond_by_audio", True)
    return sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, solver=solver, prompt_lengths=prompts, suffix_lengths=suffixes,
                                   eta=1.0 if solver == "ddim" else 0.0, seeds=torch.tensor([11, -12, 2 ** 40 + 3]), **kw)


def _forward2(eng, inputs, x, t_val, guided):
    """the step's forward, unfused: eps over [x; x] x [text; null] (or over x x text)"""
    text, null, _ = inputs
    if not guided:
        cond = eng.prepare_text_packed(text, CT)
        return eng.forward_packed(x, cond, torch.full((3,), t_val, device=DEV), CU, max_seqlen=max(LENS))
    cond = eng.prepare_text_packed(torch.cat([text, null]).contiguous(), CT + [CT[-1] + c for c in CN[1:]])
    return eng.forward_packed(x, cond, torch.full((6,), t_val, device=DEV), CU + [S + c for c in CU[1:]], max_seqlen=max(LENS))


def _chain(sg, inputs, solver, prompts, suffixes, guided_at):
    """the unfused loop: x2 after N_STEPS of forward -> window update entry; guided_at[i]: whether step i applies the guidance (the
    others run the cfg 0 entry on the conditional half, and the unconditional half is refilled before the next guided step)"""
    lib, eng = hip.lib(), sg.ditto_model.engine(torch.device("cuda:0"))
    cfg = any(guided_at)
    x2 = torch.cat([inputs[2]] * (2 if cfg else 1)).contiguous()
    q = torch.full((S, D), float("nan"), device=DEV)               # the first step must not read it
    w = torch.tensor(GUIDANCE, device=DEV)
    seeds = torch.tensor([11, -12, 2 ** 40 + 3], dtype=torch.int64, device=DEV)
    cud, qld = _i32(CU), _i32(suffixes)
    pld = None if prompts is None else _i32(prompts)
    pp = None if pld is None else pld.data_ptr()
    sched = strided_schedule(sg.alphas_cumprod, N_STEPS, 1.0) if solver == "ddim" else multistep_schedule(sg.alphas_cumprod, N_STEPS)
    stale = False
    for i, row in enumerate(sched):
        g = guided_at[i]
        if g and stale:
            x2[S:].copy_(x2[:S])
            stale = False
        x = x2 if g else x2[:S]
        eps = _forward2(eng, inputs, x, row[0], g)
        if solver == "ddim":
            t_val, a, ce, sigma = row
            co = [torch.full((3,), v, dtype=torch.float32, device=DEV) for v in (a, ce, sigma)]
            hip.check(lib.ditto_guided_update_packed_window(x.data_ptr(), eps.data_ptr(), None, seeds.data_ptr() if sigma != 0.0 else None,
                                                            t_val, w.data_ptr() if g else None, co[0].data_ptr(), co[1].data_ptr(),
                                                            co[2].data_ptr(), cud.data_ptr(), pp, qld.data_ptr(), 3, S, max(LENS), D,
                                                            int(g), _s()))
        else:
            t_val, a, kx, ke, b, gq, use_prev = row
            hip.check(lib.ditto_multistep_update_window(x.data_ptr(), eps.data_ptr(), q.data_ptr(),
                                                        C.byref(hip.MultistepCoef(a, kx, ke, b, gq, 0.0, int(use_prev), 0)), None,
                                                        w.data_ptr() if g else None, cud.data_ptr(), pp, qld.data_ptr(), 3, S, max(LENS),
                                                        D, int(g), _s()))
        stale = stale or (cfg and not g)
    return x2[:S]


def _contexts_equal(got, ref, prompts, suffixes):
    for b in range(3):
        p, qn = (0 if prompts is None else prompts[b]), suffixes[b]
        assert torch.equal(got[CU[b]:CU[b] + p], ref[CU[b]:CU[b] + p]), "the prefix rows must come back bit-equal"
        assert torch.equal(got[CU[b + 1] - qn:CU[b + 1]], ref[CU[b + 1] - qn:CU[b + 1]]), "the suffix rows must come back bit-equal"
        assert not torch.equal(got[CU[b] + p:CU[b + 1] - qn], ref[CU[b] + p:CU[b + 1] - qn])


@pytest.mark.parametrize("guided", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("prompts", [PREFIX, None], ids=["prefix_and_suffix", "suffix_only"])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_closed_call_is_the_unfused_chain_bit_for_bit(sg, inputs, solver, prompts, guided):
    with hip.batch_class(PIN):
        got = _closed(sg, inputs, solver, prompts, SUFFIX, GUIDANCE if guided else None)
        want = _chain(sg, inputs, solver, prompts, SUFFIX, [guided] * N_STEPS)
    assert got.shape == (S, D) and torch.isfinite(got).all()
    assert torch.equal(got, want), f"rel-L2 {rel_l2(got.cpu(), want.cpu()):.3e} against the unfused chain"
    _contexts_equal(got, inputs[2], prompts, SUFFIX)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_guidance_interval_is_the_chain_of_cfg1_and_cfg0_window_steps(sg, inputs, solver):
    sched = strided_schedule(sg.alphas_cumprod, N_STEPS, 0.0)
    interval = (sched[2][0], sched[1][0])                              # steps 1 and 2 guided, 0 and 3 not
    at = guided_steps(sched, interval)
    assert at == [False, True, True, False]
    with hip.batch_class(PIN):
        got = _closed(sg, inputs, solver, guidance_interval=interval)
        want = _chain(sg, inputs, solver, PREFIX, SUFFIX, at)
        full = _closed(sg, inputs, solver)
    assert torch.isfinite(got).all() and torch.equal(got, want), f"rel-L2 {rel_l2(got.cpu(), want.cpu()):.3e}"
    assert not torch.equal(got, full)
    _contexts_equal(got, inputs[2], PREFIX, SUFFIX)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_zero_suffixes_are_the_prompted_call_and_none_is_the_call_as_it_was(sg, inputs, solver):
    with hip.batch_class(PIN):
        for kw in (dict(cond_by_audio=True), dict(cond_by_audio=False)):          # x_T from audio_emb, and drawn from the seeds
            prompted = _closed(sg, inputs, solver, PREFIX, None, **kw)
            zero = _closed(sg, inputs, solver, PREFIX, [0, 0, 0], **kw)
            assert torch.isfinite(zero).all() and torch.equal(zero, prompted)
            plain = _closed(sg, inputs, solver, None, None, **kw)
            zero = _closed(sg, inputs, solver, None, [0, 0, 0], **kw)
            assert torch.equal(zero, plain)
        windowed = _closed(sg, inputs, solver, cond_by_audio=False)
        _contexts_equal(windowed, inputs[2], PREFIX, SUFFIX)
        assert not torch.equal(windowed, prompted)


# ---------------------------------------------------------------------------------------------------------------- the stream
# requests: (generated frames, prefix rows, suffix rows, text rows, n_steps).  Request 0 carries both contexts and lives through the
# arrival of 2 (a suffix only) and 3 (plain) and the retirement of 1 (a prompt only) and 2: its rows move in three regroups
REQ = [(70, 30, 25, 48, 5), (64, 20, 0, 20, 2), (40, 0, 17, 33, 2), (50, 0, 0, 7, 3)]
ARRIVALS = {0: [0, 1], 1: [2], 2: [3]}
CAPS = dict(max_rows=330, max_utterances=3, max_text_rows=256)


def _req_data():
    mk = lambda n, name, k: hash_normal((n, D), name, k) if n else None
    prefixes = [mk(p, "wss_prefix", k) for k, (_, p, _, _, _) in enumerate(REQ)]
    suffixes = [mk(q, "wss_suffix", k) for k, (_, _, q, _, _) in enumerate(REQ)]
    texts = [hash_normal((t, CFG.text_dim), "wss_text", k) for k, (_, _, _, t, _) in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, CFG.text_dim), "wss_null", k) for k in range(len(REQ))]
    return prefixes, suffixes, texts, nulls


def _solo(sg, k, data, solver):
    prefixes, suffixes, texts, nulls = data
    g, p, q, t, steps = REQ[k]
    audio = torch.zeros(p + g + q, D)
    if p:
        audio[:p] = prefixes[k]
    if q:
        audio[p + g:] = suffixes[k]
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g + q], n_steps=steps, guidance=2.0 + k,
                                  null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([900 + k]),
                                  prompt_lengths=[p] if p else None, suffix_lengths=[q] if q else None, solver=solver,
                                  eta=1.0 if solver == "ddim" else 0.0)
    assert torch.equal(out[:p].cpu(), audio[:p]) and torch.equal(out[p + g:].cpu(), audio[p + g:])
    return out[p:p + g]


def _serve(sg, data, solver, infill, which=(0, 1, 2, 3)):
    prefixes, suffixes, texts, nulls = data
    stream = sg.guided_stream(guided=True, solver=solver, infill=infill, **CAPS)
    results, handles, step, members = {}, {}, 0, []
    while step <= max(ARRIVALS) or stream.pending or stream.active:
        for k in ARRIVALS.get(step, []):
            if k not in which:
                continue
            g, p, q, t, steps = REQ[k]
            kw = dict(suffix=suffixes[k]) if q else {}
            h = stream.submit(texts[k], g, seed=900 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps,
                              eta=1.0 if solver == "ddim" else 0.0, prompt=prefixes[k], **kw)
            handles[h.id] = k
        done = stream.step()
        members.append((stream.batch.B, stream.batch.S))
        for h, out in done:
            results[handles[h.id]] = out.clone()
        step += 1
    return results, members


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_stream_requests_equal_their_solo_closed_calls(sg, solver):
    data = _req_data()
    with hip.batch_class(PIN):
        results, members = _serve(sg, data, solver, True)
        # rows in flight count P + n_frames + Q: 125 + 84, then + 57, then request 1 gone and 3 in, ...
        assert members == [(2, 209), (3, 266), (3, 232), (2, 175), (2, 175)]
        assert sorted(results) == [0, 1, 2, 3]
        for k in range(4):
            solo = _solo(sg, k, data, solver)
            assert results[k].shape == (REQ[k][0], D) and torch.isfinite(solo).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"
        # an infill stream with no suffixed request in flight gives the bits of a plain stream
        plain, _ = _serve(sg, data, solver, False, which=(1, 3))
        same, _ = _serve(sg, data, solver, True, which=(1, 3))
        for k in (1, 3):
            assert torch.equal(same[k], plain[k]) and torch.equal(plain[k], results[k])


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_steady_state_step_allocates_nothing(sg, solver):
    prefixes, suffixes, texts, nulls = _req_data()
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, solver=solver, infill=True, **CAPS)
        stream.submit(texts[0], 70, seed=900, guidance=2.0, null_text_emb=nulls[0], n_steps=8, prompt=prefixes[0], suffix=suffixes[0])
        assert stream.step() == [] and stream.step() == []
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(4):
            assert stream.step() == []
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        (h, out), = stream.drain()
    assert out.shape == (70, D) and torch.isfinite(out).all()
