"""-m gpu: the second-order multistep update over a window per utterance (csrc/guided_multistep.hip) through
ditto_multistep_update_window, in its four instantiations (CFG on / off x one step for the batch / one per utterance).

The scheme of tests/test_gpu_window_update.py: expected values come from the EXISTING ditto_multistep_update_packed run on the window
rows of x2, eps2 and q compacted into a packed batch of G_b-row utterances; the window rows of x2 (both halves) and of q must be
torch.equal.  Context rows of x2 and q hold sentinels that must survive with eps2 NaN there; with use_prev false q is NaN on the window
and must reach nothing; guard rows around every buffer catch a write outside it.  With every Q_b = 0 the call equals the existing
entry with prompt_len."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal
from test_gpu_window_update import GUARD, SHAPES, _cu, _i32, _s, window_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (a, kx, ke, b, g, use_prev): a step with a history, one without (the first), the last step's (x' = x0)
WITH, FIRST, LAST = (0.9, 1.2, -0.5, 0.4, -0.15, 1), (0.8, 1.1, -0.45, 0.3, 0.0, 0), (0.0, 1.05, -0.3, 1.0, 0.0, 0)


def _guarded(t, fill):
    g = torch.full((GUARD, t.shape[1]), fill, dtype=t.dtype, device=DEV)
    pool = torch.cat([g, t, g]).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


def _coef_table(coefs, w):
    t = torch.zeros(len(coefs), 8, dtype=torch.float32)
    for b, c in enumerate(coefs):
        t[b, :5] = torch.tensor(c[:5])
        t[b, 5] = w[b] if w is not None else 0.0
    t.view(torch.int32)[:, 6] = torch.tensor([int(c[5]) for c in coefs], dtype=torch.int32)
    return t.to(DEV)


def _call(x, eps, q, coefs, per_utt, w, cu, prompt_len, suffix_len, B, S, max_N, d, cfg_on):
    """ditto_multistep_update_window (suffix_len given) or ditto_multistep_update_packed, in place on x and q"""
    if per_utt:
        table = _coef_table(coefs, None if w is None else w.tolist())
        step, tab, wp = None, table.data_ptr(), None
    else:
        step, tab, wp = hip.MultistepCoef(*coefs[0][:5], 0.0, int(coefs[0][5]), 0), None, None if w is None else w.data_ptr()
    cud = _i32(cu)
    pld = None if prompt_len is None else _i32(prompt_len)
    head = (x.data_ptr(), eps.data_ptr(), q.data_ptr(), step, tab, wp, cud.data_ptr(), None if pld is None else pld.data_ptr())
    if suffix_len is None:
        hip.check(hip.lib().ditto_multistep_update_packed(*head, B, S, max_N, d, int(cfg_on), _s()))
    else:
        qld = _i32(suffix_len)
        hip.check(hip.lib().ditto_multistep_update_window(*head, qld.data_ptr(), B, S, max_N, d, int(cfg_on), _s()))
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def data():
    """per shape: x, eps2 = [c; u] and the history q, made once and left unchanged"""
    out = {}
    for shape, (d, npq) in SHAPES.items():
        S = sum(v[0] for v in npq)
        out[shape] = (hash_normal((S, d), "wm_x", 1).to(DEV), hash_normal((2 * S, d), "wm_eps", 2).to(DEV),
                      hash_normal((S, d), "wm_q", 3).to(DEV))
    return out


@pytest.mark.parametrize("per_utt", [False, True], ids=["one_step", "per_utt_steps"])
@pytest.mark.parametrize("coef", [WITH, FIRST], ids=["history", "first"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("shape", ["small", "stride"])
def test_windowed_update_equals_the_existing_kernel_on_the_compacted_rows(data, shape, cfg_on, coef, per_utt):
    d, npq = SHAPES[shape]
    N, P, Q = ([v[i] for v in npq] for i in range(3))
    B, S, cu = len(N), sum(N), _cu(N)
    G = [n - p - q for n, p, q in zip(N, P, Q)]
    halves = 2 if cfg_on else 1
    x, eps, q = data[shape]
    # per utterance: each at a step of its own, with and without a history side by side
    coefs = [(coef, LAST, WITH, FIRST)[b % 4] for b in range(B)] if per_utt else [coef] * B
    w = (2.0 + 0.5 * torch.arange(B, dtype=torch.float32)).to(DEV) if cfg_on else None
    gen, ctx = window_rows(cu, P, Q)
    gen2 = torch.cat([gen + h * S for h in range(halves)])
    q_start = q.clone()
    for b in range(B):                                   # no history: the window's q is NaN and must reach nothing
        if not coefs[b][5]:
            q_start[cu[b]:cu[b + 1]] = float("nan")
    # expected: the existing entry on the compacted window rows
    want_x, want_q = torch.cat([x] * halves)[gen2].contiguous(), q_start[gen].contiguous()
    _call(want_x, eps[:halves * S][gen2].contiguous(), want_q, coefs, per_utt, w, _cu(G), None, None, B, sum(G), max(G), d, cfg_on)
    # the windowed entry on the whole batch
    x_in, eps_in, q_in = torch.cat([x] * halves), eps[:halves * S].clone(), q_start.clone()
    sent = (torch.arange(len(ctx) * d, dtype=torch.float32, device=DEV).reshape(-1, d) % 97) + 1000.0
    for h in range(halves):
        x_in[ctx + h * S] = sent
        eps_in[ctx + h * S] = float("nan")
    q_in[ctx] = sent + 500.0
    x_pool, xg = _guarded(x_in, 7.0)
    eps_pool, eg = _guarded(eps_in, float("nan"))
    q_pool, qg = _guarded(q_in, 9.0)
    _call(xg, eg, qg, coefs, per_utt, w, cu, P, Q, B, S, max(N), d, cfg_on)
    assert torch.isfinite(want_x).all() and torch.isfinite(want_q).all()
    assert torch.equal(xg[gen2], want_x) and torch.equal(qg[gen], want_q)
    for h in range(halves):
        assert torch.equal(xg[ctx + h * S], sent), "a context row of x2 was written"
    assert torch.equal(qg[ctx], sent + 500.0), "a context row of q was written"
    for pool, fill in ((x_pool, 7.0), (q_pool, 9.0)):
        assert torch.all(pool[:GUARD] == fill) and torch.all(pool[-GUARD:] == fill)
    assert torch.isnan(eps_pool[:GUARD]).all() and torch.isnan(eps_pool[-GUARD:]).all()


@pytest.mark.parametrize("null_prompt", [False, True], ids=["prompt_len", "null_prompt_len"])
@pytest.mark.parametrize("per_utt", [False, True], ids=["one_step", "per_utt_steps"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_suffix_len_all_zero_is_the_existing_entry_with_prompt_len(data, cfg_on, per_utt, null_prompt):
    d, npq = SHAPES["small"]
    N, P = [v[0] for v in npq], [v[1] for v in npq]
    B, S, cu = len(N), sum(N), _cu(N)
    halves = 2 if cfg_on else 1
    x, eps, q = data["small"]
    coefs = [(WITH, LAST, WITH, FIRST)[b % 4] for b in range(B)] if per_utt else [WITH] * B
    w = (2.0 + 0.5 * torch.arange(B, dtype=torch.float32)).to(DEV) if cfg_on else None
    want_x, want_q, got_x, got_q = torch.cat([x] * halves), q.clone(), torch.cat([x] * halves), q.clone()
    e = eps[:halves * S].contiguous()
    _call(want_x, e, want_q, coefs, per_utt, w, cu, None if null_prompt else P, None, B, S, max(N), d, cfg_on)
    _call(got_x, e, got_q, coefs, per_utt, w, cu, None if null_prompt else P, [0] * B, B, S, max(N), d, cfg_on)
    assert torch.isfinite(want_x).all() and torch.equal(got_x, want_x) and torch.equal(got_q, want_q)
    assert not torch.equal(want_x, torch.cat([x] * halves))
