"""-m gpu: projected guidance through the model — SpeechGenerator.sample_guided_packed(guidance_projection=, guidance_norm_threshold=,
guidance_momentum=).

No model-level tolerance: the arithmetic is held to its fp64 reference at kernel level (test_gpu_project_kernel.py); here everything
is COMPOSITION and torch.equal, under a pinned kernel class.  A closed call with the keywords is the chain composed here step by step
— the packed forward over [x; x], ditto_guidance_project_packed on its eps, then the project update entry reading pcoef from the
scratch — for "ddim" with seeds and eta = 1, "dpmpp2m", prediction="v", prompts plus suffixes (whose rows come back bit-equal), and a
guidance interval that leaves the first step unguided (the existing unguided entry; the direction and use_prev wait);
guidance_projection=None is the call without the keyword."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import (SpeechGenerator, guided_steps, multistep_schedule, multistep_schedule_v, strided_schedule,
                                   strided_schedule_v)
from ditto_tts_amd.synth import hash_normal
from gpu_util import rel_l2
from test_gpu_stream_sampler import T_NULL, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = DiTTOConfig(256, 2, 4, 256, 256, 50)
LENS, TEXTS = (160, 64, 97, 33), (48, 20, 33, 7)
PROMPTS, SUFFIXES = (20, 0, 6, 30), (7, 5, 0, 2)   # the last: one generated row
GUIDANCE = [5.0, 2.0, 3.5, 4.0]
ETA, R, BETA = [0.0, 1.0, 0.5, 0.25], [0.5, 3.0, 1.0, 2.0], [-0.5, 0.0, -0.25, 0.3]
SEEDS = [21, 22, 23, 24]
N_STEPS = 4                                        # timesteps 49, 36, 24, 12
LATE = (0, 40)                                     # leaves the first step (t = 49) unguided
B = 4
KW = dict(guidance_projection=ETA, guidance_norm_threshold=R, guidance_momentum=BETA)


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
    return (hash_normal((CT[-1], CFG.text_dim), "pj_text", 1).to(DEV), hash_normal((CN[-1], CFG.text_dim), "pj_null", 2).to(DEV),
            hash_normal((S, D), "pj_start", 3).to(DEV))


def _closed(sg, inputs, solver, prediction="eps", prompts=None, suffixes=None, **kw):
    text, null, start = inputs
    return sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, eta=1.0 if solver == "ddim" else 0.0, seeds=torch.tensor(SEEDS),
                                   cond_by_audio=True, batch_class=B, prompt_lengths=prompts, suffix_lengths=suffixes, solver=solver,
                                   prediction=prediction, guidance=GUIDANCE, null_text_emb=null, null_text_cu_seqlens=CN, **kw)


def _chain(sg, inputs, solver, prediction, prompts, suffixes, interval):
    """the closed call composed from the forward, ditto_guidance_project_packed and the project update entries"""
    text, null, start = inputs
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    multistep, v = solver == "dpmpp2m", prediction == "v"
    x0_rows = (multistep_schedule_v if v else multistep_schedule)(sg.alphas_cumprod, N_STEPS)
    sched = x0_rows if multistep else (strided_schedule_v if v else strided_schedule)(sg.alphas_cumprod, N_STEPS, 1.0)
    mask = guided_steps(sched, interval)
    cond2 = eng.prepare_text_packed(torch.cat([text, null]).contiguous(), CT + [CT[-1] + c for c in CN[1:]])
    cond1 = eng.prepare_text_packed(text, CT)
    off2, off1 = eng.guided_offsets_packed(CU, S, N, True), eng.guided_offsets_packed(CU, S, N, False)
    opts2, opts1 = hip.CallOpts(class_rows=2 * B * N), hip.CallOpts(class_rows=B * N)
    cu2 = CU + [S + c for c in CU[1:]]
    x2 = torch.cat([start, torch.full_like(start, float("nan"))]).contiguous()
    seeds = torch.tensor(SEEDS, device=DEV)
    q = torch.full((S, D), float("nan"), device=DEV)
    direction = torch.full((S, D), float("nan"), device=DEV)
    scratch = eng.project_scratch(B, N)
    i32 = lambda t: None if t is None else torch.tensor(t, dtype=torch.int32, device=DEV)
    pl, ql = i32(prompts), i32(suffixes)
    kw = {k: t for k, t in (("prompt_len", pl), ("suffix_len", ql)) if t is not None}
    ptr = lambda t: None if t is None else t.data_ptr()
    rows = dict(cu=off2[0].data_ptr(), prompt_len=ptr(pl), suffix_len=ptr(ql), B=B, S=S, max_N=N, d=D,
                stream=torch.cuda.current_stream().cuda_stream)
    pcoefs, stale, seen = [], True, False
    for i, row in enumerate(sched):
        if not mask[i]:                                   # outside the interval: the existing unguided entry on the conditional half
            stale = True
            t = torch.full((B,), row[0], device=DEV)
            if multistep:
                eng.guided_step_packed_multistep_(x2[:S], cond1, t, B, q, hip.MultistepCoef(*row[1:6], 0.0, int(row[6]), 0), offsets=off1,
                                                  opts=opts1, **kw)
            else:
                a, ce, cz = (torch.full((B,), val, device=DEV) for val in row[1:])
                eng.guided_step_packed_(x2[:S], cond1, t, B, a, ce, cz, seeds=seeds if row[3] != 0.0 else None, step=row[0],
                                        offsets=off1, opts=opts1, **kw)
            continue
        if stale:
            x2[S:].copy_(x2[:S])
            stale = False
        proj = torch.zeros(B, 8)
        proj[:, 0], proj[:, 1] = x0_rows[i][2], x0_rows[i][3]
        for col, vals in ((2, GUIDANCE), (3, ETA), (4, R), (5, BETA)):
            proj[:, col] = torch.tensor(vals)
        proj.view(torch.int32)[:, 6] = int(seen)
        seen = True
        eps = eng.forward_packed(x2, cond2, torch.full((2 * B,), row[0], device=DEV), cu2, max_seqlen=N, opts=opts2)
        pc = eng.guidance_project_packed(x2, eps, direction, proj.to(DEV), off2[0], B, S, N, prompt_len=pl, suffix_len=ql, scratch=scratch)
        pcoefs.append(pc.clone())
        if multistep:
            hip.check(hip.call("ditto_multistep_update_packed_project", x2=x2.data_ptr(), eps2=eps.data_ptr(), q=q.data_ptr(),
                               dir=direction.data_ptr(), pcoef=pc.data_ptr(), step=hip.MultistepCoef(*row[1:6], 0.0, int(row[6]), 0),
                               coefs=None, **rows))
        else:
            a, ce, cz = (torch.full((B,), val, device=DEV) for val in row[1:])
            hip.check(hip.call("ditto_guided_update_packed_project", x2=x2.data_ptr(), eps2=eps.data_ptr(), dir=direction.data_ptr(),
                               pcoef=pc.data_ptr(), noise=None, seeds=ptr(seeds if row[3] != 0.0 else None), step=row[0], tags=None,
                               a=a.data_ptr(), ce=ce.data_ptr(), cz=cz.data_ptr(), **rows))
    return x2[:S].clone(), mask, pcoefs


CHAINS = [("ddim", "eps", False, None), ("dpmpp2m", "eps", False, None), ("ddim", "v", False, None), ("dpmpp2m", "v", True, None),
          ("ddim", "eps", True, LATE), ("dpmpp2m", "eps", False, LATE)]


@pytest.mark.parametrize("solver,prediction,context,interval", CHAINS,
                         ids=[f"{s}-{p}-{'context' if c else 'whole'}-{'interval' if i else 'every'}" for s, p, c, i in CHAINS])
@torch.no_grad()
def test_closed_call_is_the_chain_of_forward_projection_and_update(sg, inputs, solver, prediction, context, interval):
    start = inputs[2]
    prompts, suffixes = (PROMPTS, SUFFIXES) if context else (None, None)
    got = _closed(sg, inputs, solver, prediction, prompts, suffixes, guidance_interval=interval, **KW)
    want, mask, pcoefs = _chain(sg, inputs, solver, prediction, prompts, suffixes, interval)
    assert mask == ([True] * 4 if interval is None else [False, True, True, True])
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), f"rel-L2 {rel_l2(got.cpu(), want.cpu()):.3e} against the chain"
    for pc in pcoefs:                                     # the projection did something: eta = 1 alone keeps fc = 1
        assert torch.isfinite(pc).all() and float(pc[1, 1]) == 1.0 and float(pc[0, 1]) != 1.0 and float(pc[2, 1]) != 1.0, pc.tolist()
    plain = _closed(sg, inputs, solver, prediction, prompts, suffixes, guidance_interval=interval)
    assert not torch.equal(got, plain)
    if context:
        for b, (p, s) in enumerate(zip(prompts, suffixes)):
            assert torch.equal(got[CU[b]:CU[b] + p], start[CU[b]:CU[b] + p]), "the prompt rows must come back bit-equal"
            assert torch.equal(got[CU[b + 1] - s:CU[b + 1]], start[CU[b + 1] - s:CU[b + 1]]), "the suffix rows must come back bit-equal"


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_none_is_the_call_without_the_keyword(sg, inputs, solver):
    today = _closed(sg, inputs, solver, prompts=PROMPTS, suffixes=SUFFIXES)
    assert torch.isfinite(today).all()
    assert torch.equal(_closed(sg, inputs, solver, prompts=PROMPTS, suffixes=SUFFIXES, guidance_projection=None,
                               guidance_norm_threshold=None, guidance_momentum=None), today)
    # an interval without a guided step: the call without guidance, whatever the keywords say
    none = _closed(sg, inputs, solver, guidance_interval=(0, 5), **KW)
    assert torch.equal(none, _closed(sg, inputs, solver, guidance_interval=(0, 5)))


def _allocations_per_call(sg, inputs, entry, **kw):
    """the allocator's running count of allocations at the start of every guided step of one closed 2M call"""
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    seen, step = [], getattr(eng, entry)

    def spy(*a, **k):
        seen.append(torch.cuda.memory_stats()["allocation.all.allocated"])
        return step(*a, **k)

    setattr(eng, entry, spy)
    try:
        _closed(sg, inputs, "dpmpp2m", **kw)
    finally:
        delattr(eng, entry)
    assert len(seen) == N_STEPS
    return seen


@torch.no_grad()
def test_a_steady_state_step_allocates_nothing(sg, inputs):
    """the direction buffer, the table and the scratch are the call's, sized once: from the second guided step to the last the
    allocator hands out nothing — exactly as in the call without the keywords"""
    _closed(sg, inputs, "dpmpp2m", **KW)                  # warm: workspaces and rope tables exist
    plain = _allocations_per_call(sg, inputs, "guided_step_packed_multistep_")
    proj = _allocations_per_call(sg, inputs, "guided_step_packed_multistep_project_", **KW)
    print("allocations between the second and the last guided step: plain", plain[-1] - plain[1], "projected", proj[-1] - proj[1])
    assert proj[-1] - proj[1] == plain[-1] - plain[1] == 0
