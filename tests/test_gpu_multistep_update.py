"""-m gpu: the update kernel of the second-order multistep solver alone (csrc/guided_multistep.hip) through
ditto_multistep_update_packed, in its four instantiations (CFG on / off x one step for the batch / one per utterance).

Shape: d = 64, three utterances of 1, 5 and 130 rows (a single row; a partial workgroup; nine workgroups in the utterance's grid
column) with prompts of 0, 2 and 129 rows, so one utterance has a single generated row.  Expected values: the kernel's expressions in
float64 over the same fp32 inputs and fp32 coefficients (tests/multistep_ref.py), elementwise
    |got - want| <= 1e-6 (|a x| + |b x0| + |g q| + 1),
the form test_gpu_span_train.py uses for its fp32 fmaf chains.  Why it holds here: the chain is five roundings (w (c - u) + u, ke e,
kx x + ., g q, b x0 + ., a x + .), each at most 2^-24 = 6e-8 of its result; the last three are relative to terms of the bound, the
first three reach x' through b and are at most 1.8e-7 b (|kx x| + |ke e|) <= 1.8e-7 x 0.45 x (1.2 x 5 + 0.5 x 25) < 1e-6 with the
coefficients below (|b| <= 0.45, kx <= 1.2, |ke| <= 0.5, w <= 3) and |x|, |c|, |u| <= 5 — covered by the bound's constant term even
where x0 cancels.  The same count gives |q - x0| <= 1e-6 (|kx x| + |ke e| + 1).
Prompt rows of x2 and q hold sentinels that must survive bit for bit with eps2 NaN there; with use_prev false q is prefilled with NaN
and must reach nothing; guard rows around every buffer catch a write outside it."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal
from multistep_ref import update

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
D = 64
LENS, PROMPTS = (1, 5, 130), (0, 2, 129)
CU = [0, 1, 6, 136]
S, B = 136, 3
# (a, kx, ke, b, g, use_prev): a step with a history, one without (the first), the last step's (x' = x0), another with a history
WITH, FIRST, LAST, OTHER = (0.9, 1.2, -0.5, 0.4, -0.15, 1), (0.8, 1.1, -0.45, 0.3, 0.0, 0), (0.0, 1.05, -0.3, 1.0, 0.0, 0), \
    (0.95, 1.15, -0.4, 0.45, -0.2, 1)
W = [2.0, 3.0, 1.5]


def _s():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _guarded(t, fill):
    g = torch.full((GUARD, t.shape[1]), fill, dtype=t.dtype, device=DEV)
    pool = torch.cat([g, t.to(DEV), g]).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


def _coef_struct(c):
    return hip.MultistepCoef(*c[:5], 0.0, int(c[5]), 0)


def _coef_table(coefs, w):
    t = torch.zeros(len(coefs), 8, dtype=torch.float32)
    for b, c in enumerate(coefs):
        t[b, :5] = torch.tensor(c[:5])
        t[b, 5] = w[b] if w is not None else 0.0
    t.view(torch.int32)[:, 6] = torch.tensor([int(c[5]) for c in coefs], dtype=torch.int32)
    return t.to(DEV)


@pytest.fixture(scope="module")
def data():
    """the inputs, made once and left unchanged: x, eps2 = [c; u], the history q"""
    return (hash_normal((S, D), "ms_x", 1), hash_normal((2 * S, D), "ms_eps", 2), hash_normal((S, D), "ms_q", 3))


def _rows(prompts):
    gen = torch.cat([torch.arange(CU[b] + prompts[b], CU[b + 1]) for b in range(B)])
    is_p = torch.ones(S, dtype=torch.bool)
    is_p[gen] = False
    return gen, torch.nonzero(is_p).reshape(-1)


def _run(data, cfg_on, coefs, per_utt, prompts, cu=CU, prompt_arg=None):
    """one call.  coefs: one tuple per utterance (the scalar form takes coefs[0]).  Returns (x2 pool, x2, q pool, q) after the call;
    utterances without history meet NaN in q, prompt rows sentinels in x2 / q and NaN in eps2."""
    x, eps, q = data
    halves = 2 if cfg_on else 1
    gen, prm = _rows(prompts if prompts is not None else (0, 0, 0))
    x_in = torch.cat([x] * halves)
    eps_in = eps[:halves * S].clone()
    q_in = q.clone()
    for b in range(B):
        if not coefs[b][5]:
            q_in[CU[b]:CU[b + 1]] = float("nan")
    sent = (torch.arange(len(prm) * D, dtype=torch.float32).reshape(-1, D) % 97) + 1000.0
    for h in range(halves):
        x_in[prm + h * S] = sent
        eps_in[prm + h * S] = float("nan")
    q_in[prm] = sent + 500.0
    x_pool, xg = _guarded(x_in, 7.0)
    _, eg = _guarded(eps_in, float("nan"))
    q_pool, qg = _guarded(q_in, 9.0)
    w = torch.tensor(W, device=DEV) if cfg_on else None
    if per_utt:
        table = _coef_table(coefs, W if cfg_on else None)
        step, tab, wp = None, table.data_ptr(), None
    else:
        step, tab, wp = _coef_struct(coefs[0]), None, None if w is None else w.data_ptr()
    pl = prompt_arg if prompt_arg is not None else prompts
    cud, pld = _i32(cu), None if pl is None else _i32(list(pl))          # (named: they must outlive the launch)
    hip.check(hip.lib().ditto_multistep_update_packed(xg.data_ptr(), eg.data_ptr(), qg.data_ptr(), step, tab, wp, cud.data_ptr(),
                                                      None if pld is None else pld.data_ptr(), B, S, max(LENS), D, int(cfg_on), _s()))
    torch.cuda.synchronize()
    return x_pool, xg, q_pool, qg, (x_in, q_in, sent, gen, prm)


def _check(data, cfg_on, coefs, got, prompts):
    x_pool, xg, q_pool, qg, (x_in, q_in, sent, gen, prm) = got
    x, eps, q = data
    halves = 2 if cfg_on else 1
    xo, qo = xg.cpu(), qg.cpu()
    for b in range(B):
        lo, hi = CU[b] + (prompts[b] if prompts is not None else 0), CU[b + 1]
        want, x0, mag = update(x[lo:hi], eps[lo:hi], eps[S + lo:S + hi] if cfg_on else None, q[lo:hi], coefs[b], W[b] if cfg_on else None)
        for h in range(halves):
            err = (xo[h * S + lo:h * S + hi].double() - want).abs()
            assert torch.isfinite(xo[h * S + lo:h * S + hi]).all()
            assert bool((err <= 1e-6 * mag).all()), (b, h, float((err / mag).max()))
        kx, ke = (float(torch.tensor(v, dtype=torch.float32)) for v in coefs[b][1:3])
        e = (x0 - kx * x[lo:hi].double()) / ke
        err = (qo[lo:hi].double() - x0).abs()
        assert bool((err <= 1e-6 * ((kx * x[lo:hi].double()).abs() + (ke * e).abs() + 1.0)).all()), (b, float(err.max()))
    if cfg_on:
        assert torch.equal(xo[:S], xo[S:])
    for h in range(halves):                                     # prompt rows: bit-unchanged
        assert torch.equal(xo[prm + h * S], sent), "a prompt row of x2 was written"
    assert torch.equal(qo[prm], sent + 500.0), "a prompt row of q was written"
    for pool, fill in ((x_pool, 7.0), (q_pool, 9.0)):
        assert torch.all(pool[:GUARD] == fill) and torch.all(pool[-GUARD:] == fill)


@pytest.mark.parametrize("prompted", [True, False], ids=["prompts", "noprompts"])
@pytest.mark.parametrize("coef", [WITH, FIRST, LAST], ids=["history", "first", "last"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_scalar_form_against_float64(data, cfg_on, coef, prompted):
    prompts = PROMPTS if prompted else None
    coefs = [coef] * B
    _check(data, cfg_on, coefs, _run(data, cfg_on, coefs, False, prompts), prompts)


@pytest.mark.parametrize("prompted", [True, False], ids=["prompts", "noprompts"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_per_utterance_form_against_float64_each_utterance_at_its_own_step(data, cfg_on, prompted):
    """one utterance with a history between one at its first step and one at its last: their q is NaN and reaches nothing"""
    prompts = PROMPTS if prompted else None
    for coefs in ([FIRST, WITH, LAST], [OTHER, LAST, WITH]):
        _check(data, cfg_on, coefs, _run(data, cfg_on, coefs, True, prompts), prompts)


@pytest.mark.parametrize("coef", [WITH, FIRST], ids=["history", "first"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_per_utterance_form_equals_the_scalar_form_bitwise_at_a_shared_step(data, cfg_on, coef):
    coefs = [coef] * B
    a = _run(data, cfg_on, coefs, False, PROMPTS)
    b = _run(data, cfg_on, coefs, True, PROMPTS)
    gen = a[4][3]
    halves = 2 if cfg_on else 1
    assert torch.isfinite(a[1][gen]).all()
    assert torch.equal(a[1][:halves * S], b[1][:halves * S]) and torch.equal(a[3], b[3])


@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_bad_offsets_and_prompt_lengths_are_clamped(data, cfg_on):
    """cu[0] = -5 acts as 0 and cu[3] = 500 as S; prompt_len -3 acts as 0 and N_b + 70 as N_b - 1: the same result as the clamped
    values give, and no write outside the buffers (the guard rows are checked by _check)"""
    coefs = [WITH] * B
    good = _run(data, cfg_on, coefs, False, (0, 4, 129))
    bad = _run(data, cfg_on, coefs, False, (0, 4, 129), cu=[-5, 1, 6, 500], prompt_arg=(-3, 75, 200))
    _check(data, cfg_on, coefs, bad, (0, 4, 129))
    assert torch.equal(good[1], bad[1]) and torch.equal(good[3], bad[3])
