"""-m gpu: reuse of the guidance direction through the model — SpeechGenerator.sample_guided_packed(guidance_refresh=).

Under a pinned batch_class: guidance_refresh None and 1 are the call without the argument bit for bit (both solvers, prediction="v",
prompts and a suffix); guidance_refresh 2 and 3 are a loop composed HERE from sampler.refresh_plan, the engine's plain forward
(forward_packed, under the same class pins) and the stand-alone update entries ditto_guided_update_packed_reuse /
ditto_multistep_update_packed_reuse — which pins the step entries to forward + update and the sampler's loop to the plan, with and
without a guidance interval that is entered and left again.  Nothing here says anything about speech quality: the weights are
synthetic."""
import ctypes as C

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import (SpeechGenerator, guided_steps, multistep_schedule, multistep_schedule_v, refresh_plan,
                                   strided_schedule, strided_schedule_v)
from ditto_tts_amd.synth import hash_normal
from gpu_util import rel_l2
from test_gpu_stream_sampler import T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = DiTTOConfig(256, 2, 4, 256, 256, 50)
LENS, TEXTS = (96, 50, 70), (40, 7, 19)
PROMPTS, SUFFIXES = (20, 0, 9), (0, 11, 5)
GUIDANCE = [3.0, 2.0, 4.5]
SEEDS = [21, 22, 23]
N_STEPS = 6                                   # timesteps 49, 41, 32, 24, 16, 7
MIDDLE = (10, 35)                             # guided at 32, 24, 16: entered and left again
B = 3


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
    return (hash_normal((CT[-1], CFG.text_dim), "rf_text", 1).to(DEV), hash_normal((CN[-1], CFG.text_dim), "rf_null", 2).to(DEV),
            hash_normal((S, D), "rf_start", 3).to(DEV))


def _closed(sg, inputs, solver="ddim", eta=1.0, context=False, **kw):
    text, null, start = inputs
    if context:
        kw.update(prompt_lengths=PROMPTS, suffix_lengths=SUFFIXES)
    return sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, eta=eta if solver == "ddim" else 0.0, guidance=GUIDANCE,
                                   null_text_emb=null, null_text_cu_seqlens=CN, seeds=torch.tensor(SEEDS), cond_by_audio=True,
                                   batch_class=B, solver=solver, **kw)


# (solver, eta, prediction, prompts and suffixes, guidance interval)
VARIANTS = {"ddim_eta0": ("ddim", 0.0, "eps", False, None), "ddim_eta1": ("ddim", 1.0, "eps", False, None),
            "dpmpp2m": ("dpmpp2m", 0.0, "eps", False, None), "ddim_v_context": ("ddim", 1.0, "v", True, None),
            "dpmpp2m_v_context": ("dpmpp2m", 0.0, "v", True, None), "ddim_interval": ("ddim", 1.0, "eps", False, MIDDLE),
            "dpmpp2m_interval_context": ("dpmpp2m", 0.0, "v", True, MIDDLE)}


def _call(sg, inputs, variant, **kw):
    solver, eta, prediction, context, interval = VARIANTS[variant]
    return _closed(sg, inputs, solver, eta, context, prediction=prediction, guidance_interval=interval, **kw)


@pytest.fixture(scope="module")
def today(sg, inputs):
    """the calls without the new argument, computed once"""
    with torch.no_grad():
        return {v: _call(sg, inputs, v) for v in VARIANTS}


@pytest.mark.parametrize("variant", list(VARIANTS))
@torch.no_grad()
def test_refresh_none_and_one_are_the_call_without_the_argument(sg, inputs, today, variant):
    want = today[variant]
    assert torch.isfinite(want).all()
    assert torch.equal(_call(sg, inputs, variant, guidance_refresh=None), want)
    assert torch.equal(_call(sg, inputs, variant, guidance_refresh=1), want)


def _composed(sg, inputs, variant, k):
    """the loop of guidance_refresh=k from refresh_plan, forward_packed and the stand-alone reuse updates"""
    solver, eta, prediction, context, interval = VARIANTS[variant]
    text, null, start = inputs
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    lib = hip.lib()
    multistep = solver == "dpmpp2m"
    if multistep:
        sched = (multistep_schedule_v if prediction == "v" else multistep_schedule)(sg.alphas_cumprod, N_STEPS)
    else:
        sched = (strided_schedule_v if prediction == "v" else strided_schedule)(sg.alphas_cumprod, N_STEPS, eta)
    kinds, mirror = refresh_plan(guided_steps(sched, interval), k)
    cond2 = eng.prepare_text_packed(torch.cat([text, null]).contiguous(), CT + [CT[-1] + c for c in CN[1:]])
    cond1 = eng.prepare_text_packed(text, CT)
    cu2 = CU + [S + c for c in CU[1:]]
    off1 = eng.guided_offsets_packed(CU, S, N, False)
    opts2, opts1 = hip.CallOpts(class_rows=2 * B * N), hip.CallOpts(class_rows=B * N)
    x2 = torch.cat([start, torch.full_like(start, float("nan"))]).contiguous()        # the second half is refreshed before its first use
    w = torch.tensor(GUIDANCE, device=DEV)
    seeds = torch.tensor(SEEDS, device=DEV)
    q = torch.full((S, D), float("nan"), device=DEV)
    delta = torch.full((S, D), float("nan"), device=DEV)
    cud = torch.tensor(CU, dtype=torch.int32, device=DEV)
    pl = torch.tensor(PROMPTS, dtype=torch.int32, device=DEV) if context else None
    ql = torch.tensor(SUFFIXES, dtype=torch.int32, device=DEV) if context else None
    ctx = (None if pl is None else pl.data_ptr(), None if ql is None else ql.data_ptr())
    kw = dict(prompt_len=pl, suffix_len=ql) if context else {}
    stream = torch.cuda.current_stream().cuda_stream
    stale, seen = True, set()
    for i, row in enumerate(sched):
        kind = kinds[i]
        seen.add((kind, mirror[i]))
        if kind == "plain":                                  # the existing non-CFG entry on the conditional half
            t = torch.full((B,), row[0], device=DEV)
            if multistep:
                eng.guided_step_packed_multistep_(x2[:S], cond1, t, B, q, hip.MultistepCoef(*row[1:6], 0.0, int(row[6]), 0), offsets=off1,
                                                  opts=opts1, **kw)
            else:
                a, ce, cz = (torch.full((B,), v, device=DEV) for v in row[1:])
                eng.guided_step_packed_(x2[:S], cond1, t, B, a, ce, cz, seeds=seeds if row[3] != 0.0 else None, step=row[0],
                                        offsets=off1, opts=opts1, **kw)
            stale = True
            continue
        store = kind == "refresh"
        if store and stale:
            x2[S:].copy_(x2[:S])
        if store:
            eps = eng.forward_packed(x2, cond2, torch.full((2 * B,), row[0], device=DEV), cu2, N, opts=opts2)
        else:
            eps = eng.forward_packed(x2[:S], cond1, torch.full((B,), row[0], device=DEV), CU, N, opts=opts1)
        mode = hip.REUSE_STORE if store else hip.REUSE_LOAD
        if multistep:
            coef = hip.MultistepCoef(*row[1:6], 0.0, int(row[6]), 0)
            hip.check(lib.ditto_multistep_update_packed_reuse(x2.data_ptr(), eps.data_ptr(), q.data_ptr(), delta.data_ptr(), C.byref(coef),
                                                              w.data_ptr(), cud.data_ptr(), *ctx, B, S, N, D, mode, int(mirror[i]), stream))
        else:
            a, ce, cz = (torch.full((B,), v, device=DEV) for v in row[1:])
            hip.check(lib.ditto_guided_update_packed_reuse(x2.data_ptr(), eps.data_ptr(), delta.data_ptr(), None,
                                                           seeds.data_ptr() if row[3] != 0.0 else None, row[0], w.data_ptr(), a.data_ptr(),
                                                           ce.data_ptr(), cz.data_ptr(), cud.data_ptr(), *ctx, B, S, N, D, mode,
                                                           int(mirror[i]), stream))
        stale = not (store or mirror[i])
    return x2[:S].clone(), kinds, seen


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("variant", list(VARIANTS))
@torch.no_grad()
def test_refresh_k_is_the_loop_composed_from_the_plan_the_forward_and_the_updates(sg, inputs, today, variant, k):
    got = _call(sg, inputs, variant, guidance_refresh=k)
    want, kinds, seen = _composed(sg, inputs, variant, k)
    interval, context = VARIANTS[variant][4], VARIANTS[variant][3]
    if interval is None:
        assert kinds == (["refresh", "reuse"] * 3 if k == 2 else ["refresh", "reuse", "reuse"] * 2)
    else:                                                    # the first guided step behind the unguided ones is a refresh
        assert kinds == ["plain", "plain", "refresh", "reuse", "refresh" if k == 2 else "reuse", "plain"]
    assert ("reuse", True) in seen or interval is not None and k == 3
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), f"rel-L2 {rel_l2(got.cpu(), want.cpu()):.3e} against the composed loop"
    assert not torch.equal(got, today[variant]), "the reuse path did not run"
    if context:
        start = inputs[2]
        for b in range(B):
            lo, hi = CU[b], CU[b + 1]
            assert torch.equal(got[lo:lo + PROMPTS[b]], start[lo:lo + PROMPTS[b]]), "the prompt rows must come back bit-equal"
            assert torch.equal(got[hi - SUFFIXES[b]:hi], start[hi - SUFFIXES[b]:hi]), "the suffix rows must come back bit-equal"


@torch.no_grad()
def test_refusals_on_a_real_engine(sg, inputs):
    text, null, start = inputs
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        _closed(sg, inputs, guidance_refresh=2, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="guidance_refresh needs"):
        sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, seeds=torch.tensor(SEEDS), cond_by_audio=True, guidance_refresh=2)
    for bad in (0, -1, True, 2.0, "2"):
        with pytest.raises(ValueError, match="guidance_refresh"):
            _closed(sg, inputs, guidance_refresh=bad)
