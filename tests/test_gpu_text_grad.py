"""-m gpu: training for classifier-free guidance on packed batches — the gradient with respect to the text rows
(ditto_train_backward_packed_text_layers) and condition dropout with a learned null embedding (DiTTO.train_forward_packed(...,
null_text_emb=, drop=)).

Expected values come from the per-utterance fp32 oracle of tests/test_gpu_train_packed.py (its helper is copied here), with the text —
and the null embedding, where one is dropped in — as autograd leaves.  Bounds are that file's: forward rel-L2 < 2e-2, every gradient of
this chain < 3e-2 (the text gradient is one more bf16 dgrad off the same dkv); everything that is a copy, an ordered sum or a repeat is
torch.equal."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ditto_tts_amd import hip, optim
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.synth import hash_normal, synthetic_state_dict
from gpu_util import rel_l2
from oracle import ditto_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = DiTTOConfig(256, 3, 4, 256, 256, 50)
SL, TL = [200, 77, 130], [96, 40, 65]


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _build(cfg, seed):
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed))
    return m.to(DEV)


def _inputs(cfg, SL, TL, seed):
    S, S_T, B = sum(SL), sum(TL), len(SL)
    x = hash_normal((S, cfg.hidden_dim), "px", seed)
    text = hash_normal((S_T, cfg.text_dim), "ptext", seed + 1)
    t = torch.tensor([(7 * b + 3) % cfg.diffusion_steps for b in range(B)])
    target = hash_normal((S, cfg.hidden_dim), "pnoise", seed + 2)
    return x, text, t, target


def _oracle_forward_one(sd, cfg, xb, tb, tt, b, B, p, drop_seed, N_max, T_max):
    """the training forward of ONE utterance from the oracle's public pieces (O.ditto_forward would use stream 0 for every utterance)"""
    L, H = cfg.num_layers, cfg.num_heads
    temb = O.time_embedding(sd, tt)
    pos = O.rotary_table(sd["rotary.inv_freq"], xb.shape[1])
    x_skip = F.linear(xb, sd["proj_in.weight"], sd["proj_in.bias"])
    h = O.global_adaln(sd, xb, temb, tb)
    for l in range(L):
        mask = None
        if p > 0:
            mask = O.hash_dropout_mask(drop_seed, l, B, H, N_max, T_max, p)[b:b + 1, :, :xb.shape[1], :tb.shape[1]]
        h = O.dit_block(sd, f"blocks.{l}.", h, tb, pos, H, None, p, mask)
    return x_skip + F.linear(h, sd["proj_out.weight"], sd["proj_out.bias"])


def _oracle(cfg, sd_seed, x, text, t, SL, TL, target, p=0.0, drop_seed=None, null=None, drop=None, sd=None):
    """per-utterance oracle with the text (and `null`, the text of the utterances `drop` marks) as autograd leaves: loss = sum_b
    sum((out_b - target_b)^2) / (S d).  Returns (outputs [S, d], loss, parameter gradients or None with a caller's `sd`,
    text.grad [S_T, dt], null.grad or None)."""
    own = sd is None
    if own:
        sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in synthetic_state_dict(cfg, sd_seed).items()}
    text = text.clone().requires_grad_()
    null = None if null is None else null.detach().clone().requires_grad_()
    B = len(SL)
    drop = [False] * B if drop is None else [bool(v) for v in drop]
    cu, cu_t = _cu(SL), _cu(TL)
    tl_eff = [null.shape[0] if drop[b] else TL[b] for b in range(B)]
    S, d = cu[-1], cfg.hidden_dim
    outs, total = [], 0.0
    for b in range(B):
        xb = x[cu[b]:cu[b + 1]][None]
        tb = (null if drop[b] else text[cu_t[b]:cu_t[b + 1]])[None]
        ob = _oracle_forward_one(sd, cfg, xb, tb, t[b:b + 1], b, B, p, drop_seed, max(SL), max(tl_eff))
        lb = ((ob[0] - target[cu[b]:cu[b + 1]]) ** 2).sum() / (S * d)
        lb.backward()
        outs.append(ob[0].detach())
        total += float(lb.detach())
    grads = {k: v.grad for k, v in sd.items() if v.requires_grad} if own else None
    tg = text.grad if text.grad is not None else torch.zeros_like(text)
    return torch.cat(outs), total, grads, tg, None if null is None else null.grad


def _seed_of(manual):
    torch.manual_seed(manual)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


@functools.lru_cache(maxsize=None)
def _case(train_mode):
    """the d = 256 case and its oracle, computed once per mode and shared (never modified)"""
    x, text, t, target = _inputs(CFG, SL, TL, 11)
    p = 0.1 if train_mode else 0.0
    return (x, text, t, target) + _oracle(CFG, 4, x, text, t, SL, TL, target, p, _seed_of(77))


def _step(m, x, text, t, target, manual, cu_t=None, **kw):
    """one packed step on the device with text as a leaf: (eps, loss, text leaf)"""
    td = text.to(DEV).requires_grad_()
    torch.manual_seed(manual)
    out = m.train_forward_packed(x.to(DEV), _cu(SL) if cu_t is None else cu_t[0], td, _cu(TL) if cu_t is None else cu_t[1], t.to(DEV), **kw)
    loss = F.mse_loss(out, target.to(DEV))
    loss.backward()
    return out, loss, td


def _param_grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _check_text_grad(got, want, lens, tag):
    """rel-L2 over the whole tensor and per utterance (the short text's rows carry the pool term's 1 / T_b), each printed, then < 3e-2"""
    cu_t = _cu(lens)
    rs = [rel_l2(got, want)] + [rel_l2(got[cu_t[b]:cu_t[b + 1]], want[cu_t[b]:cu_t[b + 1]]) for b in range(len(lens))]
    print(f"{tag} text gradient rel_l2: whole {rs[0]:.3e}, per utterance {[f'{r:.3e}' for r in rs[1:]]}")
    assert all(r < 3e-2 for r in rs), rs
    return rs


# ----------------------------------------------------------------------------------------------- (a) against the oracle's autograd
@pytest.mark.parametrize("train_mode", [False, True])
def test_text_gradient_vs_the_oracle(train_mode):
    x, text, t, target, want_out, want_loss, want, want_text, _ = _case(train_mode)
    m = _build(CFG, 4).train(train_mode)
    out, loss, td = _step(m, x, text, t, target, 77)
    r = rel_l2(out, want_out)
    print(f"text grad train={train_mode}: forward rel_l2 {r:.3e} loss {float(loss):.6f} oracle {want_loss:.6f}")
    assert r < 2e-2 and abs(float(loss) - want_loss) < 2e-2 * want_loss
    assert td.grad is not None and td.grad.shape == text.shape and td.grad.dtype == torch.float32
    _check_text_grad(td.grad, want_text, TL, f"text grad train={train_mode}:")
    worst = max((rel_l2(p.grad, want[n]), n) for n, p in m.named_parameters() if p.grad is not None)
    print(f"text grad train={train_mode}: worst parameter gradient rel_l2 {worst[0]:.3e} ({worst[1]})")
    assert worst[0] < 3e-2
    with pytest.raises(NotImplementedError, match="detach"):                  # the dense layout keeps its refusal of text_emb ...
        m(x[:64].to(DEV)[None], text[:16].to(DEV)[None].requires_grad_(), t[:1].to(DEV))
    with pytest.raises(NotImplementedError, match="detach"):                  # ... and x's gradient stays refused here
        m.train_forward_packed(x.to(DEV).requires_grad_(), _cu(SL), text.to(DEV), _cu(TL), t.to(DEV))


# ----------------------------------------------------------------------------------------------- (b) parameter gradients untouched
def test_parameter_gradients_do_not_change_with_the_text_gradient():
    x, text, t, target = _case(True)[:4]
    res = []
    for want_text in (False, True):
        m = _build(CFG, 4).train()
        torch.manual_seed(77)
        td = text.to(DEV).requires_grad_(want_text)
        out = m.train_forward_packed(x.to(DEV), _cu(SL), td, _cu(TL), t.to(DEV))
        F.mse_loss(out, target.to(DEV)).backward()
        res.append((out.detach().clone(), _param_grads(m)))
        assert (td.grad is not None) == want_text
    assert torch.equal(res[0][0], res[1][0]) and res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 40
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


# ----------------------------------------------------------------------------------------------- (c) the backward in pieces
class _RecSync:
    def __init__(self):
        self.pieces, self.aborts, self.finishes = 0, 0, 0

    def reduce(self, piece):
        self.pieces += 1

    def abort(self):
        self.aborts += 1

    def finish(self):
        self.finishes += 1


def test_text_gradient_in_pieces_is_bitwise_the_single_call():
    x, text, t, target = _case(True)[:4]
    res = []
    for sync in (None, _RecSync()):
        m = _build(CFG, 4).train()
        m.set_grad_sync(sync, 1)
        _, _, td = _step(m, x, text, t, target, 9)
        res.append((td.grad.clone(), _param_grads(m)))
    assert (sync.pieces, sync.aborts, sync.finishes) == (3, 0, 1)              # one piece per layer
    assert torch.equal(res[0][0], res[1][0])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


# ----------------------------------------------------------------------------------------------- (d) dropout = the hand-assembled call
def test_condition_dropout_equals_the_hand_assembled_call():
    x, text, t, target = _case(True)[:4]
    T0 = 33
    null = hash_normal((T0, CFG.text_dim), "pnull", 5)
    cu_t = _cu(TL)
    # the hand-assembled text: utterance 1's rows replaced by the null rows
    hand = torch.cat([text[:cu_t[1]], null, text[cu_t[2]:]])
    TLh = [TL[0], T0, TL[2]]
    mh = _build(CFG, 4).train()
    out_h, _, hd = _step(mh, x, hand, t, target, 31, cu_t=(_cu(SL), _cu(TLh)))
    m = _build(CFG, 4).train()
    nd = torch.nn.Parameter(null.to(DEV))
    out, _, td = _step(m, x, text, t, target, 31, null_text_emb=nd, drop=[0, 1, 0])
    assert torch.equal(out, out_h)
    gh, g = _param_grads(mh), _param_grads(m)
    assert gh.keys() == g.keys() and len(g) > 40
    for n in g:
        assert torch.equal(g[n], gh[n]), n
    cu_h = _cu(TLh)
    assert torch.equal(nd.grad, hd.grad[cu_h[1]:cu_h[2]])
    assert torch.equal(td.grad[:cu_t[1]], hd.grad[:cu_h[1]]) and torch.equal(td.grad[cu_t[2]:], hd.grad[cu_h[2]:])
    assert not td.grad[cu_t[1]:cu_t[2]].any()                                   # the dropped utterance's own rows: exactly 0
    assert "null_text_emb" not in dict(m.named_parameters())
    # against the oracle, with the null embedding as a leaf
    _, _, _, want_text, want_null = _oracle(CFG, 4, x, text, t, SL, TL, target, 0.1, _seed_of(31), null=null, drop=[0, 1, 0])
    r = rel_l2(nd.grad, want_null)
    print(f"condition dropout [0,1,0]: null gradient rel_l2 {r:.3e}")
    assert r < 3e-2
    _check_text_grad(td.grad[:cu_t[1]], want_text[:cu_t[1]], TL[:1], "condition dropout [0,1,0], utterance 0:")
    # two dropped utterances: the null gradient is the fp32 sum, in utterance order, of their rows of the hand-assembled call's
    hand2 = torch.cat([null, null, text[cu_t[2]:]])
    TL2 = [T0, T0, TL[2]]
    m2h = _build(CFG, 4).train()
    _, _, h2 = _step(m2h, x, hand2, t, target, 31, cu_t=(_cu(SL), _cu(TL2)))
    m2 = _build(CFG, 4).train()
    n2 = torch.nn.Parameter(null.to(DEV))
    _, _, t2 = _step(m2, x, text, t, target, 31, null_text_emb=n2, drop=torch.tensor([True, True, False]))
    assert torch.equal(n2.grad, h2.grad[:T0] + h2.grad[T0:2 * T0])              # 0 + a + b: two fp32 adds, in order
    assert not t2.grad[:cu_t[2]].any() and torch.equal(t2.grad[cu_t[2]:], h2.grad[2 * T0:])
    _, _, _, _, want_null2 = _oracle(CFG, 4, x, text, t, SL, TL, target, 0.1, _seed_of(31), null=null, drop=[1, 1, 0])
    r2 = rel_l2(n2.grad, want_null2)
    print(f"condition dropout [1,1,0]: null gradient rel_l2 {r2:.3e}")
    assert r2 < 3e-2


# ----------------------------------------------------------------------------------------------- (e) the timed width
def test_text_gradient_at_the_timed_width_on_the_bf16_stream():
    """d = 768, 2 layers, 12 heads under hip.batch_class(32 * 1024): the bf16 tape stream, text_dim = 768 (three column tiles of the text
    GEMM), text row counts that straddle tile edges, T0 = 33, utterance 2 dropped"""
    cfg = DiTTOConfig(768, 2, 12, 256, 768, 50)
    SLw, TLw, T0, drop = [200, 130, 57, 129], [96, 130, 40, 64], 33, [0, 0, 1, 0]
    x, text, t, target = _inputs(cfg, SLw, TLw, 21)
    null = hash_normal((T0, cfg.text_dim), "pnull", 6)
    want_out, want_loss, want, want_text, want_null = _oracle(cfg, 8, x, text, t, SLw, TLw, target, 0.1, _seed_of(5), null=null,
                                                              drop=drop)
    m = _build(cfg, 8).train()
    nd = torch.nn.Parameter(null.to(DEV))
    td = text.to(DEV).requires_grad_()
    with hip.batch_class(32 * 1024):
        assert hip.full_row_plan(cfg, 1, sum(SLw)) == (True, True), "the full-row forward kernels did not engage"
        assert hip.stream_is_bf16(cfg, 1, sum(SLw)), "the bf16 stream did not engage"
        torch.manual_seed(5)
        out = m.train_forward_packed(x.to(DEV), _cu(SLw), td, _cu(TLw), t.to(DEV), null_text_emb=nd, drop=drop)
        loss = F.mse_loss(out, target.to(DEV))
        loss.backward()
    r = rel_l2(out, want_out)
    print(f"text grad d=768: forward rel_l2 {r:.3e} loss {float(loss):.6f} oracle {want_loss:.6f}")
    assert r < 2e-2 and abs(float(loss) - want_loss) < 2e-2 * want_loss
    cu_t = _cu(TLw)
    assert not td.grad[cu_t[2]:cu_t[3]].any()
    kept = [b for b in range(4) if not drop[b]]
    got = torch.cat([td.grad[cu_t[b]:cu_t[b + 1]] for b in kept])
    ref = torch.cat([want_text[cu_t[b]:cu_t[b + 1]] for b in kept])
    _check_text_grad(got, ref, [TLw[b] for b in kept], "text grad d=768:")
    rn = rel_l2(nd.grad, want_null)
    print(f"text grad d=768: null gradient rel_l2 {rn:.3e}")
    assert rn < 3e-2
    worst = max((rel_l2(p.grad, want[n]), n) for n, p in m.named_parameters() if p.grad is not None)
    print(f"text grad d=768: worst parameter gradient rel_l2 {worst[0]:.3e} ({worst[1]})")
    assert worst[0] < 3e-2


# ----------------------------------------------------------------------------------------------- (f) reproducibility and training
def test_text_and_null_gradients_are_bit_reproducible():
    x, text, t, target = _case(True)[:4]
    null = hash_normal((33, CFG.text_dim), "pnull", 5)
    res = []
    for _ in range(2):
        m = _build(CFG, 4).train()
        nd = torch.nn.Parameter(null.to(DEV))
        _, _, td = _step(m, x, text, t, target, 123, null_text_emb=nd, drop=[1, 0, 1])
        res.append((td.grad.clone(), nd.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][1].any() and res[0][0].any()


def test_training_loop_learns_the_null_embedding_and_tracks_the_oracle():
    """four fused-AdamW steps over the model's parameters plus the null embedding, drop drawn by condition_dropout_mask(B, 0.5) from a
    fixed generator, lengths changing every step: the null parameter moves, and the losses track the per-utterance oracle loop
    (torch.optim.AdamW over the oracle's weights and its own null leaf) within the 3e-2 of the packed loop test"""
    cfg = DiTTOConfig(128, 2, 2, 64, 128, 20)
    T0 = 9
    m = _build(cfg, 6).eval()
    null0 = 0.5 * hash_normal((T0, cfg.text_dim), "pnull", 7)
    nd = torch.nn.Parameter(null0.to(DEV))
    opt = optim.AdamW([p for n, p in m.named_parameters()] + [nd], lr=2e-3)
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in synthetic_state_dict(cfg, 6).items()}
    live = [v for k, v in sd.items() if v.requires_grad and ".attn.out_proj." not in k and k != "alphas_cumprod"]
    null_o = null0.clone().requires_grad_()
    opt_o = torch.optim.AdamW(live + [null_o], lr=2e-3)
    lens = [([96, 50, 130], [64, 40, 33]), ([40, 77], [20, 64]), ([100, 31, 64, 20], [10, 50, 33, 7]), ([130, 90], [60, 64])]
    gen = torch.Generator().manual_seed(3)
    losses, losses_o, dropped = [], [], 0
    for i, (SLi, TLi) in enumerate(lens):
        x, text, t, target = _inputs(cfg, SLi, TLi, 100 + 3 * i)
        drop = DiTTO.condition_dropout_mask(len(SLi), 0.5, generator=gen)
        dropped += int(drop.sum())
        out = m.train_forward_packed(x.to(DEV), _cu(SLi), text.to(DEV), _cu(TLi), t.to(DEV), null_text_emb=nd, drop=drop)
        loss = F.mse_loss(out, target.to(DEV))
        opt.zero_grad(); loss.backward(); opt.step()
        losses.append(float(loss))
        # the oracle's step: its null leaf is the optimizer's parameter itself (the helper clones it: hand the gradient over)
        opt_o.zero_grad()
        _, lo, _, _, gn = _oracle(cfg, 6, x, text, t, SLi, TLi, target, null=null_o, drop=drop.tolist(), sd=sd)
        null_o.grad = gn if gn is not None else torch.zeros_like(null_o)
        opt_o.step()
        losses_o.append(lo)
    print("condition-dropout loop losses", losses, "oracle", losses_o, "utterances dropped", dropped)
    assert dropped > 0 and int(opt.steps_applied) == 4
    assert not torch.equal(nd.detach().cpu(), null0)
    r = rel_l2(nd.detach(), null_o.detach())
    print(f"condition-dropout loop: null embedding after four steps, rel_l2 to the oracle's {r:.3e}")
    for a, b in zip(losses, losses_o):
        assert abs(a - b) < 3e-2 * b, (losses, losses_o)
