"""v-prediction on the host (no GPU): the v schedules against the eps schedules and against the float64 restatement of
tests/vpred_ref.py, the conditioning claim that motivates them, the refusals of the padded entries and the argument validation of
sample_guided_packed / guided_stream / DiTTO.span_loss_packed (all before any device work), the new symbol with its argument
refusals, and the loss kernel's DERIVED bound (vpred_ref.vloss_fp64) tried on an fp32 imitation of the kernel's arithmetic: it admits
the imitation and refuses each modelled bug."""
import math
import types

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.sampler import (SpeechGenerator, multistep_schedule, multistep_schedule_v, strided_schedule, strided_schedule_v)
from ditto_tts_amd.serving import GuidedStream
from ditto_tts_amd.synth import cosine_betas, hash_normal
from test_cabi_symbols import declared_functions
from test_stream_host import TEXT_DIM, D, StubBatch
import vpred_ref as R


def _table(T):
    """the reference's sampling table for T diffusion steps: cumprod(1 - cosine betas), fp32 as SpeechGenerator keeps it"""
    return torch.cumprod(1.0 - cosine_betas(T), dim=0)


TABLES = {T: _table(T) for T in (1000, 50)}


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("n_steps", [1, 2, 25])
@pytest.mark.parametrize("T", [1000, 50])
def test_strided_schedule_v_is_the_eps_step_on_the_recovered_eps(T, n_steps, eta):
    """Tolerance.  Both sides are float64 evaluations of the same real number.  The eps form adds a x and ce e, two terms of up to
    ~100 |x| at tau_0 (1 / alpha ~ 100) whose sum is O(|x|): its rounding error is a few 2^-53 of |a x| + |ce e|, and so are the errors
    of its coefficients (a handful of float64 operations each, none of them a cancellation).  The v form's own error is a few 2^-53
    of O(|x|), far below.  So the two agree within ~10 x 1.1e-16 x (|a x| + |ce e|); 1e-9 of that magnitude leaves six orders."""
    ac = TABLES[T]
    eps_rows, v_rows = strided_schedule(ac, n_steps, eta), strided_schedule_v(ac, n_steps, eta)
    ref = R.Strided(ac, n_steps, eta)
    g = torch.Generator().manual_seed(T + n_steps)
    x, v, z = (torch.randn(64, dtype=torch.float64, generator=g) for _ in range(3))
    assert len(v_rows) == n_steps
    for i, ((tau, a, ce, sg), (tau_v, a_v, cv, sg_v)) in enumerate(zip(eps_rows, v_rows)):
        assert tau_v == tau and sg_v == sg                              # the same timesteps, the same sigma to the bit
        ab = float(ac.double()[tau])
        al, st = math.sqrt(ab), math.sqrt(1 - ab)
        e = st * x + al * v
        want = a * x + ce * e + sg * z
        got = a_v * x + cv * v + sg * z
        scale = (a * x).abs() + (ce * e).abs()
        assert float(((got - want).abs() / scale).max()) <= 1e-9, (i, tau)
        # and the definition: x0 and eps recovered from v, then Song et al.'s eq. 12 (no coefficient form involved)
        assert float(((got - ref.step(i, x, v, z)).abs() / (x.abs() + v.abs() + 1)).max()) <= 1e-12
        assert abs(a_v) <= math.sqrt(2) and abs(cv) <= math.sqrt(2)     # a rotation-like pair at every step


def test_the_eps_form_is_ill_conditioned_where_the_v_form_is_not():
    tau, a, ce, _ = strided_schedule(TABLES[50], 25)[0]
    _, a_v, cv, _ = strided_schedule_v(TABLES[50], 25)[0]
    assert tau == 49
    assert abs(ce) > 50 and a > 50, (a, ce)                             # 1 / alpha_{T-1} ~ 100
    assert abs(a_v) <= 1.0 + 1e-12 and abs(cv) <= 1.0 + 1e-12           # eta = 0: (a_v, cv) = (cos, -sin) of the angle stepped over
    assert abs(a_v * a_v + cv * cv - 1.0) <= 1e-12


@pytest.mark.parametrize("n_steps", [1, 2, 3, 25])
@pytest.mark.parametrize("T", [1000, 50])
def test_multistep_schedule_v_changes_the_data_prediction_only(T, n_steps):
    ac = TABLES[T]
    eps_rows, v_rows = multistep_schedule(ac, n_steps), multistep_schedule_v(ac, n_steps)
    assert len(v_rows) == len(eps_rows) == n_steps
    for e, v in zip(eps_rows, v_rows):
        assert (v[0], v[1], v[4], v[5], v[6]) == (e[0], e[1], e[4], e[5], e[6])       # tau, a, b, g, use_prev: the same objects' values
        ab = float(ac.double()[e[0]])
        assert v[2] == math.sqrt(ab) and v[3] == -math.sqrt(1 - ab)
        assert abs(v[2]) <= 1 and abs(v[3]) <= 1
    # the recurrence x0 = kx x + ke out, x' = a x + b x0 + g q over every step, v form against eps form on e = sigma x + alpha v, and
    # against the restated solver.  Tolerance as above: relative to the eps form's own terms, |kx x| + |ke e| ~ 100 |x| at tau_0.
    g = torch.Generator().manual_seed(T + n_steps)
    x_e = x_v = x_r = torch.randn(64, dtype=torch.float64, generator=g)
    q_e = q_v = None
    ref = R.Multistep(ac, n_steps)
    for i, (e, v) in enumerate(zip(eps_rows, v_rows)):
        out = torch.randn(64, dtype=torch.float64, generator=g)                      # what the network returns at this step: a v
        al, st = v[2], -v[3]
        eps_e = st * x_e + al * out
        x0_e, x0_v = e[2] * x_e + e[3] * eps_e, v[2] * x_v + v[3] * out
        scale = (e[2] * x_e).abs() + (e[3] * eps_e).abs()
        assert float(((x0_v - x0_e).abs() / scale).max()) <= 1e-9, i
        nx_e = e[1] * x_e + e[4] * x0_e + (e[5] * q_e if e[6] else 0.0)
        nx_v = v[1] * x_v + v[4] * x0_v + (v[5] * q_v if v[6] else 0.0)
        x_r = ref.step(i, x_r, out)
        assert float(((nx_v - nx_e).abs() / (scale + 1)).max()) <= 1e-9, i
        assert float(((nx_v - x_r).abs() / (x_r.abs() + 1)).max()) <= 1e-9, i
        x_e, x_v, q_e, q_v = nx_e, nx_v, x0_e, x0_v


# ---------------------------------------------------------------------------------------------------------------- refusals
def _bare_generator(cfg):
    sg = object.__new__(SpeechGenerator)                          # no device: only what runs before the first GPU call
    sg.ditto_model = types.SimpleNamespace(cfg=cfg)
    return sg


def test_padded_entries_refuse_v_and_bad_values_raise():
    sg = _bare_generator(DiTTOConfig(256, 2, 4, 256, 256, 50))
    padded = (torch.zeros(1, 3, 256), torch.zeros(1, 5, 256))
    for entry in (sg.sample_guided, sg.sample_latents_strided):
        with pytest.raises(NotImplementedError, match="sample_guided_packed"):
            entry(*padded, prediction="v")
        with pytest.raises(ValueError, match="prediction"):
            entry(*padded, prediction="x0")
        with pytest.raises(NotImplementedError, match="infilling"):           # the refusals of before keep their order
            entry(*padded, prediction="v", suffix_lengths=[1])
    from ditto_tts_amd.dist import sample_sharded
    with pytest.raises(NotImplementedError, match="v-prediction"):
        sample_sharded(None, None, None, (), (), "cpu", prediction="v")
    with pytest.raises(ValueError, match="prediction"):
        sample_sharded(None, None, None, (), (), "cpu", prediction="x0")
    audio, text = torch.zeros(15, 256), torch.zeros(9, 256)
    for bad in ("x0", "V", None, 1):
        with pytest.raises(ValueError, match="prediction"):
            sg.sample_guided_packed(text, [0, 3, 6, 9], audio, [0, 5, 6, 15], prediction=bad)
        with pytest.raises(ValueError, match="prediction"):
            sg.guided_stream(max_rows=64, max_utterances=2, max_text_rows=64, prediction=bad)
        with pytest.raises(ValueError, match="prediction"):
            GuidedStream(StubBatch(), TABLES[50], guided=True, text_dim=TEXT_DIM, hidden_dim=D, max_rows=512, max_utterances=3,
                         max_text_rows=4096, prediction=bad)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_stream_requests_carry_the_v_schedule(solver):
    kw = dict(guided=True, text_dim=TEXT_DIM, hidden_dim=D, max_rows=512, max_utterances=3, max_text_rows=4096, solver=solver)
    eta = 1.0 if solver == "ddim" else 0.0
    rows = {}
    for prediction in ("eps", "v"):
        s = GuidedStream(StubBatch(), TABLES[50], prediction=prediction, **kw)
        s.submit(torch.zeros(4, TEXT_DIM), 64, seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=4, eta=eta)
        rows[prediction] = s._queue[0].schedule
        s.step()
        a = s.batch.steps[-1]
        if solver == "ddim":
            assert (a.t[0], a.a[0], a.ce[0], a.cz[0]) == tuple(rows[prediction][0])
        else:
            assert a.coef[0] == tuple(rows[prediction][0][1:])
    default = GuidedStream(StubBatch(), TABLES[50], **kw)
    assert default.prediction == "eps"
    ac = TABLES[50].double()
    if solver == "ddim":
        assert rows["eps"] == strided_schedule(ac, 4, eta) and rows["v"] == strided_schedule_v(ac, 4, eta)
    else:
        assert rows["eps"] == multistep_schedule(ac, 4) and rows["v"] == multistep_schedule_v(ac, 4)
    assert rows["v"] != rows["eps"]


def test_span_loss_packed_validates_before_any_device_work():
    m = types.SimpleNamespace()                                   # no engine, no buffers: a call that got past validation would fail on them
    loss = lambda *a, **k: DiTTO.span_loss_packed(m, *a, **k)     # noqa: E731
    pred, x0, t = torch.zeros(6, 64), torch.zeros(6, 64), torch.tensor([3, 7])
    cu, P = [0, 2, 6], [0, 1]
    kw = dict(seeds=torch.tensor([1, 2]), tag=3)
    with pytest.raises(ValueError, match="prediction"):
        loss(pred, cu, P, prediction="x0", **kw)
    for name, val in (("x0", x0), ("t", t), ("loss_weights", [1.0, 1.0])):     # they belong to "v"; eps weighting is not served
        with pytest.raises(ValueError, match=name):
            loss(pred, cu, P, **{name: val}, **kw)
        with pytest.raises(ValueError, match=name):
            loss(pred, cu, P, prediction="eps", **{name: val}, **kw)
    with pytest.raises(ValueError, match="x0="):
        loss(pred, cu, P, prediction="v", t=t, **kw)
    with pytest.raises(ValueError, match="t="):
        loss(pred, cu, P, prediction="v", x0=x0, **kw)
    for bad in ([1.0, -0.5], [1.0, float("nan")], [1.0, float("inf")], [1.0], [1.0, 2.0, 3.0], torch.tensor([1.0, -1.0]),
                torch.ones(2, 1), torch.tensor([True, False]), [True, 1.0], "11", 1.0):
        with pytest.raises(ValueError, match="loss_weights"):
            loss(pred, cu, P, prediction="v", x0=x0, t=t, loss_weights=bad, **kw)
    with pytest.raises(ValueError, match="t:"):
        loss(pred, cu, P, prediction="v", x0=x0, t=torch.tensor([3]), **kw)
    with pytest.raises(ValueError, match="x0:"):
        loss(pred, cu, P, prediction="v", x0=torch.zeros(5, 64), t=t, **kw)
    with pytest.raises(RuntimeError, match="eps is on cpu"):      # good arguments reach the device check, and only then
        loss(pred, cu, P, prediction="v", x0=x0, t=t, loss_weights=[0.0, 2.0], **kw)


def test_new_symbol_and_its_refusals():
    lib, P = hip.lib(), 4096                                      # a non-NULL pointer value: every call fails before anything reads it
    n = "ditto_span_vloss_window"
    assert n in declared_functions() and hasattr(lib, n) and n in hip.SYMBOLS
    assert lib.ditto_abi_version() == 10                          # an additive entry: the version stays
    f = lib.ditto_span_vloss_window
    ok = dict(pred=P, x0=P, noise=P, seeds=None, tag=0, ca=P, cs=P, lw=None, cu=P, pl=None, ql=None, n=64, grad=P, loss=P, ws=P,
              wsb=1 << 20, B=2, S=128, max_N=64, d=256, stream=None)
    call = lambda **k: f(*{**ok, **k}.values())                   # noqa: E731
    assert call(seeds=P) == hip.ERR_ARG and b"exactly one" in lib.ditto_last_error()          # both
    assert call(noise=None) == hip.ERR_ARG and b"exactly one" in lib.ditto_last_error()       # neither
    for name in ("pred", "x0", "ca", "cs", "cu", "grad", "loss", "ws"):
        assert call(**{name: None}) == hip.ERR_ARG, name
    assert call(d=96) == hip.ERR_SHAPE and b"d % 64" in lib.ditto_last_error()
    assert call(n=0) == hip.ERR_SHAPE and call(n=128 * 256 + 1) == hip.ERR_SHAPE
    assert call(B=0) == hip.ERR_SHAPE
    assert call(wsb=2 * 16 * 4 - 4) == hip.ERR_SIZE and b"workspace" in lib.ditto_last_error()   # 2 x ceil(64 x 256 / 1024) floats


# ---------------------------------------------------------------------------------------------------------------- the loss bound
def _case(seed=1):
    cu = R.cu_of(R.CASE_N)
    S = cu[-1]
    pred, x0 = hash_normal((S, R.CASE_D), "vp_pred", seed), hash_normal((S, R.CASE_D), "vp_x0", seed)
    z = torch.zeros(S, R.CASE_D)
    for b in range(len(R.CASE_N)):                                # Philox at the window-local index, as the kernel draws it
        lo, hi = cu[b] + R.CASE_P[b], cu[b + 1] - R.CASE_Q[b]
        z[lo:hi] = R.philox_rows(R.CASE_SEEDS[b], R.CASE_TAG, hi - lo, R.CASE_D)
    return cu, pred, x0, z


def test_the_bound_admits_an_fp32_imitation_of_the_kernel():
    cu, pred, x0, z = _case()
    for lw in (R.CASE_LW, None):
        want_loss, want_grad, bound = R.vloss_fp64(pred, x0, z, R.CASE_CA, R.CASE_CS, lw, cu, R.CASE_P, R.CASE_Q)
        gen = R.window_mask(cu, R.CASE_P, R.CASE_Q)
        assert float(bound[~gen].max()) == 0 and float(want_grad[~gen].abs().max()) == 0
        assert want_loss > 0.1 and float(want_grad.abs().max()) > 0
        for kw in (dict(z=z), dict(seeds=R.CASE_SEEDS, tag=R.CASE_TAG)):
            loss, grad = R.imitate(pred, x0, R.CASE_CA, R.CASE_CS, lw, cu, R.CASE_P, R.CASE_Q, **kw)
            ratio = R.worst_ratio(grad, want_grad, bound)
            print(f"imitation ({'weights' if lw else 'no weights'}, {list(kw)[0]}): worst ratio {ratio:.3f}, loss rel "
                  f"{abs(loss - want_loss) / want_loss:.2e}")
            assert ratio <= 1.0
            assert abs(loss - want_loss) <= R.LOSS_RTOL * want_loss
    # ca = 1, cs = 0, no weights: the imitation's target is z itself and the v loss is the MSE, bit for bit
    one, zero = [1.0] * 4, [0.0] * 4
    l_v, g_v = R.imitate(pred, x0, one, zero, None, cu, R.CASE_P, R.CASE_Q, z=z)
    df = torch.where(R.window_mask(cu, R.CASE_P, R.CASE_Q)[:, None], pred - z, torch.zeros(()))
    n_el = int(R.window_mask(cu, R.CASE_P, R.CASE_Q).sum()) * R.CASE_D
    assert torch.equal(g_v, torch.tensor(2.0 / n_el, dtype=torch.float32) * df)


@pytest.mark.parametrize("bug", ["cs_sign", "swap", "weight_loss_only", "global_philox", "suffix_grad"])
def test_the_bound_refuses_each_modelled_bug(bug):
    cu, pred, x0, z = _case()
    _, want_grad, bound = R.vloss_fp64(pred, x0, z, R.CASE_CA, R.CASE_CS, R.CASE_LW, cu, R.CASE_P, R.CASE_Q)
    kw = dict(seeds=R.CASE_SEEDS, tag=R.CASE_TAG) if bug == "global_philox" else dict(z=z)
    _, grad = R.imitate(pred, x0, R.CASE_CA, R.CASE_CS, R.CASE_LW, cu, R.CASE_P, R.CASE_Q, bug=bug, **kw)
    ratio = R.worst_ratio(grad, want_grad, bound)
    print(f"{bug}: worst ratio {ratio:.3e}")
    assert ratio > 100.0
