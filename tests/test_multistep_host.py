"""The second-order multistep solver on the host (no GPU): sampler.multistep_schedule against the float64 restatement and against the
closed-form Gaussian problem (its error below DDIM's at equal steps, and at 12 steps below DDIM's at 25), its first-order ends,
the argument refusals, the stream's bookkeeping (each request at its own index of its own schedule, use_prev false at its own first
step, the history segment of a survivor) and the new symbols."""
import types

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator, multistep_schedule, strided_schedule
from ditto_tts_amd.serving import _DST_Q, _SRC_Q, GuidedStream, history_segment
from ditto_tts_amd.synth import cosine_betas
from multistep_ref import Solver, gaussian_eps, gaussian_exact
from test_cabi_symbols import declared_functions
from test_stream_host import GUIDANCE, R, TEXT_DIM, D, StubBatch, _acp

NEW = ("ditto_multistep_update_packed", "ditto_guided_step_packed_multistep_opts")
P = 4096   # a non-NULL pointer value: every call below fails its argument checks before anything touches it


@pytest.fixture(scope="module")
def table():
    return torch.cumprod(1 - cosine_betas(1000), 0)


def _errors(table, n, s2):
    """(DDIM's, 2M's) relative error of the final sample on data ~ N(0, s2), float64, from x_T = 1 (the problem is linear in x_T)"""
    acd = table.double()
    x = 1.0
    for t, a, ce, _ in strided_schedule(table, n, 0.0):
        x = a * x + ce * gaussian_eps(x, float(acd[t]), s2)
    y, q = 1.0, 0.0
    for t, a, kx, ke, b, g, use_prev in multistep_schedule(table, n):
        x0 = kx * y + ke * gaussian_eps(y, float(acd[t]), s2)
        y, q = a * y + b * x0 + (g * q if use_prev else 0.0), x0
    exact = gaussian_exact(1.0, float(acd[-1]), s2)
    return abs(x - exact) / abs(exact), abs(y - exact) / abs(exact)


@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_solver_error_on_the_closed_form_gaussian_problem(table, s2):
    err = {n: _errors(table, n, s2) for n in (10, 12, 20, 25)}
    for n, (ddim, two_m) in err.items():
        print(f"s2 {s2} n {n}: DDIM {ddim:.3e}  2M {two_m:.3e}")
        assert two_m < ddim, (s2, n, ddim, two_m)
    assert err[12][1] < err[25][0], (s2, err[12][1], err[25][0])


def test_a_wrong_history_term_fails_the_solver_error_check(table):
    """the check above has teeth: the history weight with the other sign, or doubled, loses to DDIM somewhere"""
    acd = table.double()
    for scale in (-1.0, 2.0):
        lost = False
        for s2 in (0.25, 1.0, 4.0):
            y, q = 1.0, 0.0
            for t, a, kx, ke, b, g, use_prev in multistep_schedule(table, 12):
                x0 = kx * y + ke * gaussian_eps(y, float(acd[t]), s2)
                y, q = a * y + (b + (1 - scale) * g) * x0 + (scale * g * q if use_prev else 0.0), x0
            exact = gaussian_exact(1.0, float(acd[-1]), s2)
            lost |= abs(y - exact) / abs(exact) >= _errors(table, 25, s2)[0]
        assert lost, scale


@pytest.mark.parametrize("T,n_steps", [(1000, 1), (1000, 2), (1000, 12), (1000, 25), (50, 7), (50, 50)])
def test_schedule_is_the_restatement_and_its_ends_are_first_order(T, n_steps):
    ac = torch.cumprod(1 - cosine_betas(T), 0)
    sched = multistep_schedule(ac, n_steps)
    ddim = strided_schedule(ac, n_steps, 0.0)
    assert [s[0] for s in sched] == [s[0] for s in ddim]
    # step 0 (and a one-step schedule): first-order data prediction is DDIM
    _, a, kx, ke, b, g, use_prev = sched[0]
    assert not use_prev and g == 0.0
    assert a + b * kx == pytest.approx(ddim[0][1], rel=1e-12) and b * ke == pytest.approx(ddim[0][2], rel=1e-12)
    # the last step lands on x0
    assert sched[-1][1:2] + sched[-1][4:] == (0.0, 1.0, 0.0, False)
    assert [s[6] for s in sched] == [0 < i < n_steps - 1 for i in range(n_steps)]
    # against the restatement in the paper's form, along one trajectory with an arbitrary eps
    ref = Solver(ac, n_steps)
    x = y = torch.tensor([0.7, -1.3], dtype=torch.float64)
    q = torch.zeros(2, dtype=torch.float64)
    for i, (t, a, kx, ke, b, g, use_prev) in enumerate(sched):
        eps = torch.sin(3.0 * x + i)
        x0 = kx * x + ke * eps
        x, q = a * x + b * x0 + (g * q if use_prev else 0.0), x0
        y = ref.step(i, y, torch.sin(3.0 * y + i))
        assert torch.allclose(x, y, rtol=1e-9, atol=1e-9), (i, x, y)
    for bad in (0, T + 1):
        with pytest.raises(ValueError):
            multistep_schedule(ac, bad)


def _bare_generator(cfg):
    sg = object.__new__(SpeechGenerator)                          # no device: only what runs before the first GPU call
    sg.ditto_model = types.SimpleNamespace(cfg=cfg)
    return sg


def test_argument_refusals():
    sg = _bare_generator(DiTTOConfig(256, 2, 4, 256, 256, 50))
    audio, text = torch.zeros(15, 256), torch.zeros(9, 256)
    packed = (text, [0, 3, 6, 9], audio, [0, 5, 6, 15])
    with pytest.raises(ValueError, match="deterministic"):
        sg.sample_guided_packed(*packed, solver="dpmpp2m", eta=1.0)
    with pytest.raises(ValueError, match="deterministic"):
        sg.sample_guided_packed(*packed, solver="dpmpp2m", noises=[torch.zeros(15, 256)])
    for entry in (sg.sample_guided_packed, ):
        with pytest.raises(ValueError, match="solver"):
            entry(*packed, solver="dpmpp3m")
    padded = (torch.zeros(1, 3, 256), torch.zeros(1, 5, 256))
    for entry in (sg.sample_guided, sg.sample_latents_strided):
        with pytest.raises(NotImplementedError, match="sample_guided_packed"):
            entry(*padded, solver="dpmpp2m")
        with pytest.raises(ValueError, match="solver"):
            entry(*padded, solver="euler")
    with pytest.raises(ValueError, match="solver"):
        sg.guided_stream(max_rows=64, max_utterances=1, max_text_rows=8, solver="euler")
    with pytest.raises(ValueError, match="solver"):
        GuidedStream(StubBatch(), _acp(), max_rows=64, max_utterances=1, max_text_rows=8, guided=False, text_dim=TEXT_DIM, hidden_dim=D,
                     solver="euler")
    s = _stream()
    with pytest.raises(ValueError, match="eta must be 0"):
        s.submit(torch.zeros(4, TEXT_DIM), 64, seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=4, eta=1.0)
    assert s.pending == 0


def _stream(guided=True):
    return GuidedStream(StubBatch(), _acp(), guided=guided, text_dim=TEXT_DIM, hidden_dim=D, max_rows=512, max_utterances=3,
                        max_text_rows=4096, solver="dpmpp2m")


@pytest.mark.parametrize("guided", [True, False])
def test_stream_bookkeeping_under_staggered_submission(guided):
    """the scenario of test_stream_host.py: every request at its own index of its own multistep_schedule, use_prev false at its own
    first step and its own last step, whatever its neighbours do"""
    s = _stream(guided)
    arrivals = {0: [0, 1], 2: [2], 3: [3, 4]}
    step = 0
    while step == 0 or s.pending or s.active:
        for k in arrivals.get(step, []):
            n, t, steps = R[k]
            kw = dict(guidance=GUIDANCE[k], null_text_emb=torch.zeros(5, TEXT_DIM)) if guided else {}
            s.submit(torch.zeros(t, TEXT_DIM), n, seed=100 + k, n_steps=steps, **kw)
        s.step()
        step += 1
    assert step == 11
    acp = _acp()
    index = {i: 0 for i in range(5)}
    first_seen = {}
    for n_step, a in enumerate(s.batch.steps):
        assert a.a is None and a.ce is None and a.cz is None and a.tags is None
        for j, x in enumerate(a.handles):
            i = x.id
            first_seen.setdefault(i, n_step)
            sched = multistep_schedule(acp, R[i][2])
            assert (a.t[j],) + a.coef[j] == sched[index[i]]
            assert a.coef[j][5] == (0 < index[i] < R[i][2] - 1)
            if guided:
                assert a.w[j] == GUIDANCE[i]
            index[i] += 1
    assert index == {i: R[i][2] for i in range(5)}
    assert first_seen == {0: 0, 1: 0, 2: 2, 3: 4, 4: 6}           # requests 2, 3 and 4 start while others are mid-schedule
    assert sorted(s._schedules) == [(4, 0.0), (5, 0.0), (6, 0.0), (8, 0.0)]
    # a survivor's history moves with it: its generated rows, from where the last regroup put it
    r = types.SimpleNamespace(row=204, P=30, n_frames=90)
    d4 = D // 4
    assert history_segment(r, 140, d4) == [hip.REGROUP_COPY, _SRC_Q, _DST_Q, 0, 234 * d4, 170 * d4, 90 * d4, 0]
    assert (_SRC_Q, _DST_Q) == (5, 4) and hip.REGROUP_BUFS == 6


def test_new_symbols_and_their_refusals():
    lib = hip.lib()
    names = declared_functions()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in hip.SYMBOLS
    assert lib.ditto_abi_version() == 10
    import ctypes as C
    assert C.sizeof(hip.MultistepCoef) == 32
    co = hip.MultistepCoef(1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0, 0)

    def upd(x2=P, eps2=P, q=P, step=co, coefs=None, w=P, cu=P, B=2, S=128, max_N=64, d=256, cfg=1):
        return lib.ditto_multistep_update_packed(x2, eps2, q, None if step is None else C.byref(step), coefs, w, cu, None, B, S, max_N, d,
                                                 cfg, None)

    for kw, code, word in [(dict(x2=None), hip.ERR_ARG, b"null"), (dict(q=None), hip.ERR_ARG, b"null"), (dict(cu=None), hip.ERR_ARG, b"null"),
                           (dict(step=None), hip.ERR_ARG, b"exactly one"), (dict(coefs=P), hip.ERR_ARG, b"exactly one"),
                           (dict(w=None), hip.ERR_ARG, b"needs w"), (dict(step=None, coefs=P + 8), hip.ERR_ARG, b"aligned"),
                           (dict(B=0), hip.ERR_SHAPE, b"positive"), (dict(d=96), hip.ERR_SHAPE, b"% 64")]:
        assert upd(**kw) == code, kw
        assert word in lib.ditto_last_error(), (kw, lib.ditto_last_error())
    assert lib.ditto_guided_step_packed_multistep_opts(None, P, P, P, P, P, None, P, C.byref(co), None, P, 2, 128, 64, 8, 8, 1, P, P, P,
                                                       1 << 20, None, None) == hip.ERR_ARG
