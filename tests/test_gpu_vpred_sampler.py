"""-m gpu: v-prediction through the model — SpeechGenerator.sample_guided_packed(prediction="v") and guided_stream(prediction="v").

(a) the closed call against a Python loop that calls forward_packed itself (over [x; x] x [text; null] under guidance) on the float32
    image of its own float64 state and applies the float64 v update of tests/vpred_ref.py — x0 and eps recovered from v, then the
    solver's definition; no coefficient form of ditto_tts_amd/sampler.py — per utterance within the loop tolerance of
    test_gpu_multistep_sampler.py and test_gpu_guided_sampler.py (rel-L2 <= 2e-2).  Configurations: ddim, eta 0, x_T from seeds; dpmpp2m
    with guidance; ddim with guidance, guidance_rescale and prompt_lengths; ddim, eta 1, seeded z, guidance, prompt_lengths and
    suffix_lengths.  (guidance_rescale with suffix_lengths is refused by sample_guided_packed — the statistics have no windowed form —
    so the two travel in separate runs.)  Context rows come back bit-equal to the input.
(b) a request stream under a pinned class: every request, one of which joins mid-flight, is torch.equal to the closed call of it
    alone, both solvers.
(c) boundedness, the point of the parameterisation: with the synthetic weights, 50 steps and the same seeds, max |x| over the v
    loop's trajectory stays within a small multiple of max |x_T| (measured 2.96 x), while the eps loop's leaves 1e3 (measured 5.5e5):
    see test_v_trajectory_stays_bounded_where_the_eps_trajectory_does_not.
Measured rel-L2 of (a) on an MI355X: 6e-4 .. 3.4e-3 over the four configurations."""
import numpy as np
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.synth import hash_normal
from ditto_tts_amd.varlen import pack
from gpu_util import rel_l2
from rescale_ref import reference as rescale_reference
from test_gpu_stream_sampler import SMALL, T_NULL, _model
from test_gpu_window_train import _philox_buffer
import vpred_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = SMALL                                        # DiTTO(256, 2, 4, 256, 256, 50)
LENS, TEXTS = (70, 64, 129), (48, 20, 33)
PROMPTS, SUFFIXES = (30, 0, 100), (8, 20, 0)
GUIDANCE = [3.0, 2.0, 4.5]
PHI = [0.7, 0.0, 0.3]
SEEDS = [21, 22, 23]
N_STEPS = 4
PIN = 4096
B = 3
CU, CT, CN = R.cu_of(LENS), R.cu_of(TEXTS), R.cu_of([T_NULL] * B)
S, D, N = CU[-1], CFG.hidden_dim, max(LENS)
TOL = 2e-2                                         # test_gpu_multistep_sampler.py (b): the loop tolerance against a float64 restatement


@pytest.fixture(scope="module")
def sg():
    return SpeechGenerator(ditto_model=_model(CFG, seed=3), device=DEV)


@pytest.fixture(scope="module")
def inputs():
    return (hash_normal((CT[-1], CFG.text_dim), "vps_text", 1).to(DEV), hash_normal((CN[-1], CFG.text_dim), "vps_null", 2).to(DEV),
            hash_normal((S, D), "vps_start", 3).to(DEV))


def _network(eng, inputs, y, t_val, guided):
    """the network's output at the float32 image of the float64 state y: (conditional, unconditional or None), float64"""
    text, null, _ = inputs
    yf = y.float()
    if not guided:
        cond = eng.prepare_text_packed(text, CT)
        return eng.forward_packed(yf.contiguous(), cond, torch.full((B,), t_val, device=DEV), CU, max_seqlen=N).double(), None
    cond = eng.prepare_text_packed(torch.cat([text, null]).contiguous(), CT + [CT[-1] + c for c in CN[1:]])
    out = eng.forward_packed(torch.cat([yf, yf]).contiguous(), cond, torch.full((2 * B,), t_val, device=DEV),
                             CU + [S + c for c in CU[1:]], max_seqlen=N).double()
    return out[:S], out[S:]


def _reference(sg, inputs, start, solver, eta, guidance, prompts, suffixes, phi, seeds):
    """the float64 loop: forward_packed, CFG and (optionally) the rescale on the v outputs, vpred_ref's update on the window rows"""
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    P, Q = prompts or (0,) * B, suffixes or (0,) * B
    gen = R.window_mask(CU, P, Q).to(DEV)[:, None]
    ref = R.Multistep(sg.alphas_cumprod.cpu(), N_STEPS) if solver == "dpmpp2m" else R.Strided(sg.alphas_cumprod.cpu(), N_STEPS, eta)
    y = start.double()
    for i, t_val in enumerate(ref.taus):
        c, u = _network(eng, inputs, y, t_val, guidance is not None)
        v = c
        if guidance is not None:
            v = torch.cat([R.guided(c[CU[b]:CU[b + 1]], u[CU[b]:CU[b + 1]], guidance[b]) for b in range(B)])
            if phi is not None:                    # Lin et al. section 3.4 on the outputs as they are, over the generated rows
                for b in range(B):
                    lo, hi = CU[b] + P[b], CU[b + 1]
                    s = rescale_reference(c[lo:hi].cpu().numpy().astype(np.float32), u[lo:hi].cpu().numpy().astype(np.float32),
                                          guidance[b], phi[b])["s"]
                    v[CU[b]:CU[b + 1]] *= s
        if solver == "dpmpp2m":
            new = ref.step(i, y, v)
        else:
            z = None
            if ref.sigma(i) != 0.0:
                z = torch.nan_to_num(_philox_buffer(eng, list(LENS), list(P), list(Q), D, seeds, t_val)).double()
            new = ref.step(i, y, v, z)
        y = torch.where(gen, new, y)               # the context rows are never updated
    return y


CONFIGS = {
    "ddim-seeds": dict(solver="ddim", eta=0.0, guidance=None, prompts=None, suffixes=None, phi=None, x_T="seeds"),
    "dpmpp2m-cfg": dict(solver="dpmpp2m", eta=0.0, guidance=GUIDANCE, prompts=None, suffixes=None, phi=None, x_T="audio"),
    "ddim-cfg-rescale-prompts": dict(solver="ddim", eta=0.0, guidance=GUIDANCE, prompts=PROMPTS, suffixes=None, phi=PHI, x_T="audio"),
    "ddim-eta1-cfg-window": dict(solver="ddim", eta=1.0, guidance=GUIDANCE, prompts=PROMPTS, suffixes=SUFFIXES, phi=None, x_T="audio"),
}


@pytest.mark.parametrize("name", list(CONFIGS))
@torch.no_grad()
def test_closed_call_against_the_float64_v_loop_on_the_same_forwards(sg, inputs, name):
    c = CONFIGS[name]
    text, null, start = inputs
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device=DEV)
    kw = dict(guidance=c["guidance"], null_text_emb=null, null_text_cu_seqlens=CN) if c["guidance"] is not None else {}
    with hip.batch_class(PIN):
        got = sg.sample_guided_packed(text, CT, start, CU, n_steps=N_STEPS, eta=c["eta"], seeds=seeds, cond_by_audio=c["x_T"] == "audio",
                                      prompt_lengths=c["prompts"], suffix_lengths=c["suffixes"], solver=c["solver"],
                                      guidance_rescale=c["phi"], prediction="v", **kw)
        if c["x_T"] == "seeds":                    # what the call starts from: ditto_noise_normal(seeds, 0xFFFFFFFF), packed
            xt = torch.empty(B, N, D, dtype=torch.float32, device=DEV)
            eng.noise_normal_(xt, seeds, 0xFFFFFFFF)
            x_T = pack(xt, list(LENS))[0]
        else:
            x_T = start
        want = _reference(sg, inputs, x_T, c["solver"], c["eta"], c["guidance"], c["prompts"], c["suffixes"], c["phi"], seeds)
    assert got.shape == (S, D) and torch.isfinite(got).all()
    P, Q = c["prompts"] or (0,) * B, c["suffixes"] or (0,) * B
    for b in range(B):
        lo, hi = CU[b] + P[b], CU[b + 1] - Q[b]
        r = rel_l2(got[lo:hi].cpu(), want[lo:hi].cpu())
        print(f"{name} utterance {b}: rel-L2 {r:.3e} against the float64 v loop")
        assert r <= TOL, f"utterance {b}: rel-L2 {r:.3e}"
        assert torch.equal(got[CU[b]:lo], start[CU[b]:lo]) and torch.equal(got[hi:CU[b + 1]], start[hi:CU[b + 1]]), \
            "the context rows must come back bit-equal"


# ---------------------------------------------------------------------------------------------------------------- the stream
# requests: (generated frames, prompt rows, text rows, n_steps).  Request 1 retires after step 2; request 2 joins after step 1
REQ = [(70, 0, 48, 4), (64, 0, 20, 2), (99, 30, 33, 3)]
ARRIVALS = {0: [0, 1], 1: [2]}
CAPS = dict(max_rows=330, max_utterances=3, max_text_rows=256)


def _req_data():
    prompts = [hash_normal((p, D), "vpst_prompt", k) if p else None for k, (_, p, _, _) in enumerate(REQ)]
    texts = [hash_normal((t, CFG.text_dim), "vpst_text", k) for k, (_, _, t, _) in enumerate(REQ)]
    nulls = [hash_normal((T_NULL, CFG.text_dim), "vpst_null", k) for k in range(len(REQ))]
    return prompts, texts, nulls


def _solo(sg, k, data, solver, prediction="v"):
    prompts, texts, nulls = data
    g, p, t, steps = REQ[k]
    audio = torch.zeros(p + g, D)
    if p:
        audio[:p] = prompts[k]
    out = sg.sample_guided_packed(texts[k].to(DEV), [0, t], audio.to(DEV), [0, p + g], n_steps=steps, eta=1.0 if solver == "ddim" else 0.0,
                                  guidance=2.0 + k, null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL],
                                  seeds=torch.tensor([700 + k]), prompt_lengths=[p] if p else None, solver=solver,
                                  prediction=prediction)
    return out[p:]


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@torch.no_grad()
def test_stream_requests_equal_their_solo_closed_calls_bit_for_bit(sg, solver):
    data = _req_data()
    prompts, texts, nulls = data
    with hip.batch_class(PIN):
        stream = sg.guided_stream(guided=True, solver=solver, prediction="v", **CAPS)
        results, handles, step, members = {}, {}, 0, []
        while step == 0 or stream.pending or stream.active:
            for k in ARRIVALS.get(step, []):
                g, p, t, steps = REQ[k]
                h = stream.submit(texts[k], g, seed=700 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps,
                                  eta=1.0 if solver == "ddim" else 0.0, prompt=prompts[k])
                handles[h.id] = k
            done = stream.step()
            members.append(stream.batch.B)
            for h, out in done:
                results[handles[h.id]] = out.clone()
            step += 1
        assert step == 4 and members == [2, 3, 2, 2] and sorted(results) == [0, 1, 2]          # request 2 joined mid-flight
        for k in range(3):
            solo = _solo(sg, k, data, solver)
            assert results[k].shape == (REQ[k][0], D) and torch.isfinite(solo).all()
            assert torch.equal(results[k], solo), f"request {k}: rel-L2 {rel_l2(results[k].cpu(), solo.cpu()):.3e} against its solo run"
        assert not torch.equal(results[0], _solo(sg, 0, data, solver, prediction="eps"))       # the stream did run the v schedule


# ---------------------------------------------------------------------------------------------------------------- boundedness
V_MEASURED = 2.961       # max |x| over the v trajectory / max |x_T|, measured on an MI355X


@torch.no_grad()
def test_v_trajectory_stays_bounded_where_the_eps_trajectory_does_not(sg, inputs):
    """50 steps (every timestep of the 50-entry table), eta 0, no guidance, the same seeds; max |x| after every step, recorded by a
    wrapper around the engine's step entry.  Measured on an MI355X: max |x_T| = 4.424; v loop max |x| = 13.100 (ratio 2.961);
    eps loop max |x| = 5.487e+05.  The v side is asserted against 10 x the measured ratio (margin for other
    clocks and kernel classes; nothing rests on it but the order of magnitude), the eps side only as > 1e3."""
    text, _, start = inputs
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device=DEV)
    entry = eng.guided_step_packed_
    peaks = {}

    def run(prediction):
        trace = []

        def recorded(x2, *a, **k):
            if not trace:
                trace.append(float(x2.abs().max()))          # x_T
            out = entry(x2, *a, **k)
            trace.append(float(x2.abs().max()))
            return out

        eng.guided_step_packed_ = recorded
        try:
            sg.sample_guided_packed(text, CT, start, CU, n_steps=50, eta=0.0, seeds=seeds, prediction=prediction)
        finally:
            del eng.guided_step_packed_
        assert len(trace) == 51
        peaks[prediction] = (trace[0], max(trace))

    run("v")
    run("eps")
    (xt_v, peak_v), (xt_e, peak_e) = peaks["v"], peaks["eps"]
    print(f"max |x_T| {xt_v:.3f}; v loop max |x| {peak_v:.3f} (ratio {peak_v / xt_v:.3f}); eps loop max |x| {peak_e:.4e}")
    assert xt_v == xt_e
    assert np.isfinite(peak_v) and peak_v / xt_v <= 10 * V_MEASURED
    assert peak_e > 1e3
