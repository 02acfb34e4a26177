"""ditto_tts_amd.optim.AdamW on small models (d = 256, 2 layers; the loop test's d = 128): one step from real gradients against
torch's chain — clip_grad_norm_, torch.optim.AdamW, lerp_ — run in float64 on clones, inside the bounds of tests/optim_ref.py; the
forward after step() sees the new weights with no invalidate(); the four-step loop of test_gpu_train_packed.py with this optimizer;
the state dict round trip and a torch.optim.AdamW state dict; ema_weights() / ema_state_dict(); no host synchronisation and no device
allocation in a steady-state step; the same step twice gives the same bits."""
import copy

import pytest
import torch
import torch.nn.functional as F

import optim_ref as R
from ditto_tts_amd import hip, optim
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.synth import hash_normal, synthetic_inputs, synthetic_state_dict
from test_gpu_train_packed import _build, _cu, _inputs, _oracle_packed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = DiTTOConfig(256, 2, 4, 256, 256, 50)
B_, N_, T_ = 2, 96, 40
LR, WD, DECAY = 2e-3, 1e-2, 0.99


def _batch(seed=3):
    x, text, t = synthetic_inputs(CFG, B_, N_, T_, seed=seed)
    return x.to(DEV), text.to(DEV), t.to(DEV), hash_normal((B_, N_, CFG.hidden_dim), "noise", seed + 1).to(DEV)


def _backward(m, seed=3):
    x, text, t, target = _batch(seed)
    m.zero_grad(set_to_none=True)
    F.mse_loss(m(x, text, t), target).backward()


def _live(m):
    return [(n, p) for n, p in m.named_parameters() if p.grad is not None]


def _fake_grads(m, seed):
    """fixed gradients of the size of real ones on every parameter that gets one (everything but .attn.out_proj.*)"""
    gen = torch.Generator().manual_seed(seed)
    for n, p in m.named_parameters():
        p.grad = None if ".attn.out_proj." in n else (1e-2 * torch.randn(p.shape, generator=gen)).to(DEV)


def _snapshot(m, opt):
    out = {}
    for n, p in m.named_parameters():
        st = opt.state.get(p, {})
        out[n] = (p.detach().clone(),) + tuple(st[k].clone() for k in ("exp_avg", "exp_avg_sq", "ema") if k in st)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert len(a[n]) == len(b[n]) and all(torch.equal(x, y) for x, y in zip(a[n], b[n])), n


def _forward(m, rows=B_ * N_):
    x, text, t, _ = _batch(11)
    with torch.no_grad(), hip.batch_class(rows):
        return m(x, text, t)


def _fresh_from(sd):
    f = DiTTO(CFG.hidden_dim, CFG.num_layers, CFG.num_heads, CFG.time_dim, CFG.text_dim, CFG.diffusion_steps)
    f.load_state_dict(sd)
    return f.to(DEV).eval()


def test_one_step_against_torchs_chain_in_float64_and_the_next_forward_sees_it():
    m = _build(CFG, 1).eval()
    _backward(m)
    live = _live(m)
    assert len(live) == len(list(m.named_parameters())) - 2 * CFG.num_layers        # .attn.out_proj.* get no gradient
    grads = [p.grad for _, p in live]
    norm = R.global_norm([g.cpu() for g in grads])
    max_norm = 0.5 * norm                                                          # an input: half the norm, so the step clips
    # torch's chain, float64, on clones
    p64 = [torch.nn.Parameter(p.detach().double().clone()) for _, p in live]
    for q, g in zip(p64, grads):
        q.grad = g.double().clone()
    ema64 = [q.detach().clone() for q in p64]
    total = torch.nn.utils.clip_grad_norm_(p64, max_norm, foreach=False)
    topt = torch.optim.AdamW(p64, lr=LR, weight_decay=WD, foreach=False)
    topt.step()
    with torch.no_grad():
        for e, q in zip(ema64, p64):
            e.lerp_(q, 1.0 - DECAY)
    before = [p.detach().clone() for _, p in live]
    opt = optim.AdamW(m.parameters(), lr=LR, weight_decay=WD, max_norm=max_norm, ema_decay=DECAY)
    y_old = _forward(m)
    opt.step()
    n_el = sum(g.numel() for g in grads)
    gn, cc = float(opt.grad_norm), float(opt.clip_coef)
    assert abs(gn - norm) <= (R.norm_rtol(n_el) + R.U32) * norm and abs(float(total) - norm) <= 1e-12 * norm
    assert abs(cc - 0.5) <= 1e-6 and int(opt.skipped_steps) == 0 and int(opt.steps_applied) == 1
    clip = R.clip_factor(norm, max_norm)
    worst = {}
    for (name, p), p0, g, q, e in zip(live, before, grads, p64, ema64):
        z = torch.zeros_like(p0)
        want, bound = R.chain_fp64(p0, g, z, z, p0, 1, LR, WD, eps=1e-8, decay=DECAY, clip=clip)
        st, ts = opt.state[p], topt.state[q]
        for key, got, chain in (("p", p.detach(), q.detach()), ("m", st["exp_avg"], ts["exp_avg"]), ("v", st["exp_avg_sq"], ts["exp_avg_sq"]),
                                ("ema", st["ema"], e)):
            assert torch.allclose(want[key], chain, rtol=1e-10, atol=1e-16), (name, key)     # the restatement IS torch's chain
            r = R.worst_ratio(got, chain.cpu(), bound[key].cpu())
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, f"{name}: {key} at {r:.3f} of its bound"
    print("one step against torch's chain: worst ratio to the bound", worst)
    # the forward right after step(): the new weights, no invalidate()
    y_new = _forward(m)
    assert not torch.equal(y_new, y_old)
    assert torch.equal(y_new, _forward(_fresh_from(m.state_dict())))


def test_training_loop_meets_the_packed_loop_tests_bar():
    """test_gpu_train_packed.py's four-step loop (lengths change every step) with this optimizer, clip and EMA off: the losses track
    the per-utterance oracle loop (torch.optim.AdamW on the oracle's own weights) within that test's 3e-2."""
    cfg = DiTTOConfig(128, 2, 2, 64, 128, 20)
    m = _build(cfg, 6).eval()
    opt = optim.AdamW([p for n, p in m.named_parameters()], lr=2e-3)
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in synthetic_state_dict(cfg, 6).items()}
    live = [v for k, v in sd.items() if v.requires_grad and ".attn.out_proj." not in k and k != "alphas_cumprod"]
    opt_o = torch.optim.AdamW(live, lr=2e-3)
    lens = [([96, 50, 130], [64, 40, 33]), ([40, 77], [20, 64]), ([100, 31, 64, 20], [10, 50, 33, 7]), ([130, 90], [60, 64])]
    losses, losses_o = [], []
    for i, (SL, TL) in enumerate(lens):
        x, text, t, target = _inputs(cfg, SL, TL, 100 + 3 * i)
        loss = F.mse_loss(m.train_forward_packed(x.to(DEV), _cu(SL), text.to(DEV), _cu(TL), t.to(DEV)), target.to(DEV))
        opt.zero_grad(); loss.backward(); opt.step()
        losses.append(float(loss))
        opt_o.zero_grad()
        _, lo, _ = _oracle_packed(cfg, 6, x, text, t, SL, TL, target, sd=sd)
        opt_o.step()
        losses_o.append(lo)
    print("fused-optimizer loop losses", losses, "oracle", losses_o)
    assert int(opt.steps_applied) == 4
    for a, b in zip(losses, losses_o):
        assert abs(a - b) < 3e-2 * b, (losses, losses_o)


def test_state_dict_round_trip_and_a_torch_adamw_state_dict():
    kw = dict(lr=LR, weight_decay=WD, max_norm=0.05, skip_nonfinite=True, ema_decay=DECAY)
    a = _build(CFG, 2).eval()
    oa = optim.AdamW(a.parameters(), **kw)
    for s in (1, 2):
        _fake_grads(a, s)
        oa.step()
    sd_opt, sd_model = copy.deepcopy(oa.state_dict()), {k: v.clone() for k, v in a.state_dict().items()}
    assert set(sd_opt) == {"state", "param_groups", "skipped_steps"}
    entry = next(iter(sd_opt["state"].values()))
    assert tuple(entry) == ("step", "exp_avg", "exp_avg_sq", "ema") and float(entry["step"]) == 2.0
    _fake_grads(a, 3)
    oa.step()
    b = _fresh_from(sd_model)
    ob = optim.AdamW(b.parameters(), **kw)
    ob.load_state_dict(sd_opt)
    _fake_grads(b, 3)
    ob.step()
    _same(_snapshot(a, oa), _snapshot(b, ob))
    assert int(ob.steps_applied) == 3 and float(ob.grad_norm) == float(oa.grad_norm)
    # a checkpoint of torch.optim.AdamW: loads, and the next step continues it
    c = _build(CFG, 2).eval()
    params = [p for n, p in c.named_parameters() if ".attn.out_proj." not in n]
    topt = torch.optim.AdamW(params, lr=LR, weight_decay=WD)
    _fake_grads(c, 1)
    topt.step()
    oc = optim.AdamW(params, lr=LR, weight_decay=WD)
    oc.load_state_dict(topt.state_dict())
    assert int(oc.steps_applied) == 1
    _fake_grads(c, 2)
    before = {p: (p.detach().clone(), topt.state[p]["exp_avg"].clone(), topt.state[p]["exp_avg_sq"].clone(), p.grad) for p in params}
    oc.step()
    for p, (p0, m0, v0, g) in before.items():
        want, bound = R.chain_fp64(p0, g, m0, v0, None, 2, LR, WD, eps=1e-8)
        for key, got in (("p", p.detach()), ("m", oc.state[p]["exp_avg"]), ("v", oc.state[p]["exp_avg_sq"])):
            assert R.worst_ratio(got, want[key].cpu(), bound[key].cpu()) <= 1.0, key


def test_ema_weights_scope_and_ema_state_dict():
    m = _build(CFG, 4).eval()
    opt = optim.AdamW(m.parameters(), lr=5e-2, weight_decay=WD, ema_decay=0.9)
    for s in (1, 2):
        _fake_grads(m, s)
        opt.step()
    trained = {n: p.detach().clone() for n, p in m.named_parameters()}
    y_trained = _forward(m)
    want = _forward(_fresh_from(opt.ema_state_dict(m)))
    with opt.ema_weights():
        y_ema = _forward(m)
        name, p = next((n, p) for n, p in m.named_parameters() if p in opt.state)
        assert torch.equal(opt.state[p]["ema"], trained[name])          # inside the scope the buffers hold the TRAINED weights
    assert torch.equal(y_ema, want) and not torch.equal(y_ema, y_trained)
    for n, p in m.named_parameters():
        assert torch.equal(p, trained[n]), n
    assert torch.equal(_forward(m), y_trained)                          # and the engine is back on them, with no invalidate()
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("inside")
    for n, p in m.named_parameters():
        assert torch.equal(p, trained[n]), n


def test_steady_state_step_does_not_synchronise_or_allocate():
    m = _build(CFG, 5).eval()
    opt = optim.AdamW(m.parameters(), lr=LR, weight_decay=WD, max_norm=1.0, skip_nonfinite=True, ema_decay=DECAY)
    _fake_grads(m, 1)
    opt.step()                                          # the first step creates state, table and scratch
    torch.cuda.set_sync_debug_mode("error")             # probe once: does this build raise on a synchronising call?
    try:
        torch.ones(1, device=DEV).item()
        honoured = False
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("set_sync_debug_mode('error') honoured by this build:", honoured)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in (2, 3):
            for p in m.parameters():                    # new gradient VALUES in the same tensors: a backward allocates, step() must not
                if p.grad is not None:
                    p.grad.mul_(0.5)
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert int(opt.steps_applied) == 3 and int(opt.skipped_steps) == 0


def test_the_same_step_twice_gives_the_same_bits():
    snaps = []
    for _ in range(2):
        m = _build(CFG, 7).eval()
        opt = optim.AdamW(m.parameters(), lr=LR, weight_decay=WD, max_norm=0.05, ema_decay=DECAY)
        for s in (1, 2):
            _fake_grads(m, s)
            opt.step()
        snaps.append((_snapshot(m, opt), float(opt.grad_norm), float(opt.clip_coef)))
    _same(snaps[0][0], snaps[1][0])
    assert snaps[0][1:] == snaps[1][1:] and snaps[0][2] < 1.0
