"""-m gpu: training on PACKED variable-length batches (DiTTO.train_forward_packed / train_forward, the packed training attention
kernels, the per-utterance GlobalAdaLN backward).

The oracle has no notion of lengths: the expected values are built PER UTTERANCE — fp32 autograd of oracle/ditto_oracle.py on that
utterance's slice alone with loss sum((out_b - target_b)^2) / (S d), gradients summed over the utterances.  In train mode the forward is
composed from the oracle's public pieces so that utterance b gets ITS slice of the hash keep-mask (stream b H + h, local indices).
Tolerances are those tests/test_gpu_train.py states for the same quantities on the same kernels: forward rel-L2 <= 2e-2, per-tensor
parameter gradient < 3e-2, kernel-level attention forward < 1.5e-2, dq / dk / dv < 2e-2."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import attn_train_fwd_ref as F_REF
from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.synth import hash_normal, synthetic_state_dict
from gpu_util import bf16, max_abs, rel_l2, stream
from oracle import ditto_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


# ----------------------------------------------------------------------------------------------- kernel level
def _heads(t, S, H, dh):
    return t.view(S, H, dh).permute(1, 0, 2)


def _unrope(g, pos):   # g [H, S, 64], pos [S, 64] = cat(freqs, freqs): the transpose of O.apply_rope's rotation
    return g * pos.cos() - O.rotate_half(g) * pos.sin()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("self_attn,QL,KL,H", [
    (False, [40, 100, 128, 70], [1, 72, 64, 130], 2),     # shorter than a tile, mid-tile end, whole tiles, Skv = 1
    (False, [64, 130], [650, 33], 1),                      # >= 10 key tiles: the four-buffer ring wraps
    (False, [710, 20], [64, 90], 1),                       # >= 11 query tiles for the dk,dv kernel's ring
    (True, [40, 192, 100, 257], None, 2),                  # self-attention: cu_q = cu_kv, RoPE backward fused
    (True, [704, 33], None, 1),
])
def test_packed_attention_forward_and_backward_vs_autograd(self_attn, QL, KL, H, p):
    """ditto_attention_train_packed_bf16 / ditto_attention_bwd_packed_bf16 against fp32 torch on the same bf16-rounded operands, one
    utterance at a time: O, log-sum-exp, dq, dk, dv.  The buffers carry slack rows past S (and dq / dk / dv / O / lse start as a
    sentinel): nothing outside every utterance's range is written."""
    lib = hip.lib()
    dh, SLACK, SENT = 64, 96, 1024.0   # (exact in bf16)
    KL = QL if self_attn else KL
    B, d = len(QL), H * dh
    cq, ck = _cu(QL), _cu(KL)
    Sq, Skv = cq[-1], ck[-1]
    seed, layer, scale = 0x1234567890ABCDEF, 3, dh ** -0.5
    q = bf16(hash_normal((Sq, d), "q", 1)).float()
    k = bf16(hash_normal((Skv, d), "k", 2)).float()
    v = bf16(hash_normal((Skv, d), "v", 3)).float()
    do = bf16(hash_normal((Sq, d), "do", 4)).float()
    mask = O.hash_dropout_mask(seed, layer, B, H, max(QL), max(KL), p) if p > 0 else None
    pos = O.rotary_table(O.rotary_inv_freq(dh), max(QL))
    want_o, want_lse = torch.zeros(Sq, d), torch.zeros(H, Sq)
    want_dq, want_dk, want_dv = torch.zeros(Sq, d), torch.zeros(Skv, d), torch.zeros(Skv, d)
    for b in range(B):
        qs, ks = slice(cq[b], cq[b + 1]), slice(ck[b], ck[b + 1])
        nq, nk = QL[b], KL[b]
        qb, kb, vb = (z.clone().requires_grad_(True) for z in (q[qs], k[ks], v[ks]))
        qh, kh, vh = _heads(qb, nq, H, dh), _heads(kb, nk, H, dh), _heads(vb, nk, H, dh)
        s = torch.matmul(qh, kh.transpose(-2, -1)) * scale
        a = torch.softmax(s, dim=-1)
        if mask is not None:
            a = a * mask[b, :, :nq, :nk] / (1.0 - p)
        ob = torch.matmul(a, vh).permute(1, 0, 2).reshape(nq, d)
        ob.backward(do[qs])
        want_o[qs] = ob.detach()
        want_lse[:, qs] = torch.logsumexp(s.detach(), dim=-1) / 0.6931471805599453
        gq, gk = qb.grad, kb.grad
        if self_attn:
            # the kernel is handed the ROTATED q / k (the QKV epilogue's output) and returns the gradient with respect to the
            # unrotated ones: R^T g = g cos - rotate_half(g) sin at the row's position inside its utterance
            gq = _unrope(_heads(gq, nq, H, dh), pos[:nq]).permute(1, 0, 2).reshape(nq, d)
            gk = _unrope(_heads(gk, nk, H, dh), pos[:nk]).permute(1, 0, 2).reshape(nk, d)
        want_dq[qs], want_dk[ks], want_dv[ks] = gq, gk, vb.grad

    def pad(t, fill=0.0):
        return torch.cat([t, torch.full((SLACK,) + tuple(t.shape[1:]), fill, dtype=t.dtype)]).contiguous()
    qd, kd, vd, dod = (bf16(pad(z)).to(DEV) for z in (q, k, v, do))
    cqd = torch.tensor(cq, dtype=torch.int32, device=DEV)
    ckd = cqd if self_attn else torch.tensor(ck, dtype=torch.int32, device=DEV)
    o = torch.full((Sq + SLACK, d), SENT, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((H, Sq + SLACK), SENT, dtype=torch.float32, device=DEV)
    # lse is [H, q_rows]: hand the kernel q_rows = Sq + SLACK so that the slack columns exist in every head's row
    RQ, RK = Sq + SLACK, Skv + SLACK
    hip.check(lib.ditto_attention_train_packed_bf16(qd.data_ptr(), d, kd.data_ptr(), d, vd.data_ptr(), d, o.data_ptr(), d,
                                                    lse.data_ptr(), cqd.data_ptr(), ckd.data_ptr(), B, H, RQ, RK, max(QL), max(KL), dh,
                                                    scale, p, seed, layer, stream()))
    r = rel_l2(o[:Sq].float(), want_o)
    print(f"packed attention fwd self={self_attn} p={p}: O rel_l2 {r:.3e}")
    assert r < 1.5e-2
    assert max_abs(lse[:, :Sq], want_lse) < 2e-3 * (1 + float(want_lse.abs().max()))
    # ... and every slot within the elementwise bound derived from the kernel's arithmetic (attn_train_fwd_ref.py)
    ref = F_REF.reference(SimpleNamespace(q=bf16(q), k=bf16(k), v=bf16(v), segs=F_REF.packed_segs(QL, KL), H=H, scale=scale, p=0.0,
                                          keep=None))
    r = F_REF.worst_ratio(lse[:, :Sq].cpu(), ref.L, ref.e_L)
    print(f"lse worst ratio against the elementwise bound: {r:.3f} (bound at most {float(ref.e_L.max()):.3e} log2 units)")
    assert r <= 1.0 and float(ref.e_L.max()) <= 2.0 ** -7
    assert torch.all(o[Sq:].float() == SENT) and torch.all(lse[:, Sq:] == SENT)
    nb = lib.ditto_attention_bwd_packed_workspace_bytes(B, H, RQ)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dq = torch.full((RQ, d), SENT, dtype=torch.bfloat16, device=DEV)
    dk = torch.full((RK, d), SENT, dtype=torch.bfloat16, device=DEV)
    dv = torch.full((RK, d), SENT, dtype=torch.bfloat16, device=DEV)
    rc, rs = (None, None)
    if self_attn:
        half = pos[:, :dh // 2]
        rc, rs = torch.cos(half).contiguous().to(DEV), torch.sin(half).contiguous().to(DEV)
    hip.check(lib.ditto_attention_bwd_packed_bf16(qd.data_ptr(), d, kd.data_ptr(), d, vd.data_ptr(), d, dod.data_ptr(), d, o.data_ptr(), d,
                                                  lse.data_ptr(), dq.data_ptr(), d, dk.data_ptr(), d, dv.data_ptr(), d, cqd.data_ptr(),
                                                  ckd.data_ptr(), B, H, RQ, RK, max(QL), max(KL), dh, scale, p, seed, layer,
                                                  None if rc is None else rc.data_ptr(), None if rs is None else rs.data_ptr(),
                                                  ws.data_ptr(), nb, stream()))
    for name, got, want, n in (("dq", dq, want_dq, Sq), ("dk", dk, want_dk, Skv), ("dv", dv, want_dv, Skv)):
        r = rel_l2(got[:n].float(), want)
        print(f"packed attention bwd self={self_attn} p={p}: {name} rel_l2 {r:.3e}")
        assert r < 2e-2, f"{name}: rel-L2 {r:.3e}"
        assert torch.all(got[n:].float() == SENT), f"{name}: rows outside every utterance were written"


# ----------------------------------------------------------------------------------------------- whole model
def _build(cfg, seed):
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed))
    return m.to(DEV)


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


def _oracle_packed(cfg, sd_seed, x, text, t, SL, TL, target, p=0.0, drop_seed=None, sd=None):
    """per-utterance oracle: outputs [S, d], loss = sum_b sum((out_b - target_b)^2) / (S d), gradients summed over b"""
    own = sd is None
    if own:
        sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in synthetic_state_dict(cfg, sd_seed).items()}
    cu, cu_t = _cu(SL), _cu(TL)
    S, d = cu[-1], cfg.hidden_dim
    outs, total = [], 0.0
    for b in range(len(SL)):
        xb, tb = x[cu[b]:cu[b + 1]][None], text[cu_t[b]:cu_t[b + 1]][None]
        ob = _oracle_forward_one(sd, cfg, xb, tb, t[b:b + 1], b, len(SL), p, drop_seed, max(SL), max(TL))
        lb = ((ob[0] - target[cu[b]:cu[b + 1]]) ** 2).sum() / (S * d)
        lb.backward()
        outs.append(ob[0].detach())
        total += float(lb)
    grads = {k: v.grad for k, v in sd.items() if v.requires_grad} if own else None
    return torch.cat(outs), total, grads


def _check_grads(m, want, tol, tag=""):
    worst = (0.0, "")
    for name, p in m.named_parameters():
        if ".attn.out_proj." in name:
            assert p.grad is None, f"{name}: the reference never uses it, so it must get no gradient"
            continue
        assert p.grad is not None, f"{name}: no gradient"
        r = rel_l2(p.grad, want[name])
        worst = max(worst, (r, name))
    print(f"{tag} worst gradient rel_l2 {worst[0]:.3e} ({worst[1]})")
    for name, p in m.named_parameters():
        if ".attn.out_proj." not in name:
            r = rel_l2(p.grad, want[name])
            assert r < tol, f"{name}: rel-L2 {r:.3e}"
    return worst


def _inputs(cfg, SL, TL, seed):
    S, S_T, B = sum(SL), sum(TL), len(SL)
    x = hash_normal((S, cfg.hidden_dim), "px", seed)
    text = hash_normal((S_T, cfg.text_dim), "ptext", seed + 1)
    t = torch.tensor([(7 * b + 3) % cfg.diffusion_steps for b in range(B)])
    target = hash_normal((S, cfg.hidden_dim), "pnoise", seed + 2)
    return x, text, t, target


@pytest.mark.parametrize("train_mode", [False, True])
def test_packed_model_vs_per_utterance_oracle(train_mode):
    """d = 256, 3 layers, 4 heads, SL = [200, 77, 130], TL = [96, 40, 65]: forward, loss and every gradient"""
    cfg = DiTTOConfig(256, 3, 4, 256, 256, 50)
    SL, TL = [200, 77, 130], [96, 40, 65]
    x, text, t, target = _inputs(cfg, SL, TL, 11)
    p = 0.1 if train_mode else 0.0
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    want_out, want_loss, want = _oracle_packed(cfg, 4, x, text, t, SL, TL, target, p, seed)
    m = _build(cfg, 4)
    m.train(train_mode)
    torch.manual_seed(77)
    out = m.train_forward_packed(x.to(DEV), _cu(SL), text.to(DEV), _cu(TL), t.to(DEV))
    r = rel_l2(out, want_out)
    print(f"packed model train={train_mode}: forward rel_l2 {r:.3e}")
    assert out.requires_grad and out.shape == (sum(SL), 256) and r < 2e-2
    loss = F.mse_loss(out, target.to(DEV))
    loss.backward()
    print(f"packed model train={train_mode}: loss {float(loss):.6f} oracle {want_loss:.6f}")
    assert abs(float(loss) - want_loss) < 2e-2 * want_loss
    _check_grads(m, want, 3e-2, f"packed model train={train_mode}:")


def test_packed_model_at_the_timed_width_on_the_bf16_stream():
    """d = 768, 2 layers, 12 heads under hip.batch_class(32 * 1024): the full-row forward and the bf16 tape stream engage; train mode,
    lengths that straddle 128-row tiles, a duplicate timestep (the t_embedding scatter must accumulate)"""
    cfg = DiTTOConfig(768, 2, 12, 256, 768, 50)
    SL, TL = [200, 130, 57, 129], [96, 130, 40, 64]
    x, text, t, target = _inputs(cfg, SL, TL, 21)
    t[0] = t[-1]
    torch.manual_seed(5)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    want_out, want_loss, want = _oracle_packed(cfg, 8, x, text, t, SL, TL, target, 0.1, seed)
    m = _build(cfg, 8).train()
    with hip.batch_class(32 * 1024):
        # (the training step puts its tape on the bf16 stream exactly where both fused launches take the 128-row full-row kernel)
        assert hip.full_row_plan(cfg, 1, sum(SL)) == (True, True), "the full-row forward kernels did not engage"
        assert hip.stream_is_bf16(cfg, 1, sum(SL)), "the bf16 stream did not engage"
        torch.manual_seed(5)
        out = m.train_forward_packed(x.to(DEV), _cu(SL), text.to(DEV), _cu(TL), t.to(DEV))
        loss = F.mse_loss(out, target.to(DEV))
        loss.backward()
    r = rel_l2(out, want_out)
    print(f"packed d=768: forward rel_l2 {r:.3e} loss {float(loss):.6f} oracle {want_loss:.6f}")
    assert r < 2e-2 and abs(float(loss) - want_loss) < 2e-2 * want_loss
    _check_grads(m, want, 3e-2, "packed d=768:")


@pytest.mark.parametrize("cfg,pin", [(DiTTOConfig(256, 2, 4, 256, 256, 50), 4096), (DiTTOConfig(768, 2, 12, 256, 768, 50), 32 * 1024)])
def test_forward_invariance_alone_or_among_neighbours(cfg, pin):
    """eval mode, pinned class: an utterance's eps rows are torch.equal whether it is packed alone or first among neighbours"""
    SL, TL = [200, 130, 57], [96, 130, 40]
    x, text, t, _ = _inputs(cfg, SL, TL, 31)
    m = _build(cfg, 3).eval()
    with hip.batch_class(pin):
        full = m.train_forward_packed(x.to(DEV), _cu(SL), text.to(DEV), _cu(TL), t.to(DEV)).detach()
        alone = m.train_forward_packed(x[:SL[0]].to(DEV), [0, SL[0]], text[:TL[0]].to(DEV), [0, TL[0]], t[:1].to(DEV)).detach()
        x2, text2, _, _ = _inputs(cfg, [SL[0], 64, 300], [TL[0], 33, 70], 41)
        x2[:SL[0]], text2[:TL[0]] = x[:SL[0]], text[:TL[0]]
        t2 = torch.tensor([int(t[0]), 9, 1])
        other = m.train_forward_packed(x2.to(DEV), _cu([SL[0], 64, 300]), text2.to(DEV), _cu([TL[0], 33, 70]), t2.to(DEV)).detach()
    assert torch.equal(full[:SL[0]], alone) and torch.equal(other[:SL[0]], alone)


@pytest.mark.parametrize("cfg,SL,TL", [(DiTTOConfig(256, 2, 4, 256, 256, 50), [512, 300, 700, 536], [256, 100, 200, 77]),
                                       (DiTTOConfig(768, 2, 12, 256, 768, 50), [1024, 900, 1148], [128, 100, 70])])
def test_packed_gradients_are_bit_reproducible(cfg, SL, TL):
    """the same packed step twice (train mode, fixed seed; split-K weight gradients, and at d = 768 with 3072 rows the fused gated
    backward): bitwise the same gradients — no atomics, per-utterance partials reduced in a fixed order"""
    x, text, t, target = (z.to(DEV) for z in _inputs(cfg, SL, TL, 51))
    grads = []
    for _ in range(2):
        m = _build(cfg, 9).train()
        torch.manual_seed(123)
        F.mse_loss(m.train_forward_packed(x, _cu(SL), text, _cu(TL), t), target).backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 40
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


def test_backward_in_pieces_is_bitwise_the_single_call():
    cfg = DiTTOConfig(256, 3, 4, 256, 256, 50)
    SL, TL = [200, 77, 130], [96, 40, 65]
    x, text, t, target = (z.to(DEV) for z in _inputs(cfg, SL, TL, 61))

    class Rec:
        def __init__(self): self.pieces = []
        def reduce(self, piece): self.pieces.append(len(piece))
        def finish(self): pass
        def abort(self): pass
    res = []
    for sync in (None, Rec()):
        m = _build(cfg, 2).train()
        m.set_grad_sync(sync, 1)
        torch.manual_seed(9)
        F.mse_loss(m.train_forward_packed(x, _cu(SL), text, _cu(TL), t), target).backward()
        res.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    assert len(sync.pieces) == 3 and sum(sync.pieces) == len(res[1])     # one piece per layer; every gradient in exactly one
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), n


def test_padded_convenience_equals_the_packed_call():
    cfg = DiTTOConfig(256, 2, 4, 256, 256, 50)
    SL, TL = [200, 77, 130], [96, 40, 65]
    B, N, T, d = 3, 208, 100, 256
    xp, tp, t, target = (z.to(DEV) for z in _inputs(cfg, SL, TL, 71))
    cu, cu_t = _cu(SL), _cu(TL)

    def padded(fill):
        x = torch.full((B, N, d), fill, device=DEV)
        tx = torch.full((B, T, d), fill, device=DEV)
        for b in range(B):
            x[b, :SL[b]] = xp[cu[b]:cu[b + 1]]
            tx[b, :TL[b]] = tp[cu_t[b]:cu_t[b + 1]]
        return x, tx
    m = _build(cfg, 7).train()
    torch.manual_seed(3)
    out_p = m.train_forward_packed(xp, cu, tp, cu_t, t)
    F.mse_loss(out_p, target, reduction="sum").backward()
    gp = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    valid = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    tgt = torch.zeros(B, N, d, device=DEV)
    for b in range(B):
        valid[b, :SL[b]] = True
        tgt[b, :SL[b]] = target[cu[b]:cu[b + 1]]
    for fill, junk in ((0.0, 0.0), (float("nan"), 0.0), (0.0, 1e3)):
        m.zero_grad(set_to_none=True)
        x, tx = padded(fill)
        torch.manual_seed(3)
        out = m.train_forward(x, tx, t, speech_lengths=SL, text_lengths=TL)
        assert out.shape == (B, N, d) and torch.all(out[~valid] == 0)
        assert torch.equal(out[valid], out_p)
        # gradient placed on padded rows (junk) changes nothing: the loss reads the padded rows with a weight
        w = torch.where(valid[..., None], torch.ones((), device=DEV), torch.full((), junk, device=DEV))
        loss = (((out - tgt) ** 2) * torch.where(valid[..., None], 1.0, 0.0)).sum() + (out * w * (~valid[..., None])).sum()
        loss.backward()
        for n, p in m.named_parameters():
            if p.grad is not None:
                assert torch.equal(p.grad, gp[n]), (fill, junk, n)


def test_training_loop_with_changing_lengths_tracks_the_oracle_and_stops_allocating():
    """four AdamW steps on packed batches whose lengths change every step track the per-utterance oracle loop's losses within 3e-2
    relative (the bound of test_training_closure_like_the_reference).  Tapes and workspace are pooled by capacity: after one step at
    the largest S / S_T every later step runs on THAT tape and THAT workspace (same address, same size, one buffer in the pool — a
    pool keyed by (B, S, S_T) would hold one tape per shape), and the allocator's counter moves by the same number of allocations
    per step whatever the lengths (outputs and gradients are allocated per step; a tape never is)."""
    cfg = DiTTOConfig(128, 2, 2, 64, 128, 20)
    m = _build(cfg, 6).eval()
    opt = torch.optim.AdamW([p for n, p in m.named_parameters()], lr=2e-3)
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in synthetic_state_dict(cfg, 6).items()}
    live = [v for k, v in sd.items() if v.requires_grad and ".attn.out_proj." not in k and k != "alphas_cumprod"]
    opt_o = torch.optim.AdamW(live, lr=2e-3)
    lens = [([96, 50, 130], [64, 40, 33]), ([40, 77], [20, 64]), ([100, 31, 64, 20], [10, 50, 33, 7]), ([130, 90], [60, 64])]
    # capacity first: one throw-away forward + backward at the largest S / S_T (weights untouched: no optimizer step)
    x, text, t, target = _inputs(cfg, [140, 140], [80, 80], 99)
    F.mse_loss(m.train_forward_packed(x.to(DEV), [0, 140, 280], text.to(DEV), [0, 80, 160], t.to(DEV)), target.to(DEV)).backward()
    m.zero_grad(set_to_none=True)
    eng = m.engine(train=True)      # (the engine of the parameters' own device: the one the forwards above ran on)

    def buffers():
        pool = eng._tapes["packed"]
        assert len(pool) == 1, f"{len(pool)} tapes in the pool: one per shape, not one by capacity"
        return pool[0].data_ptr(), pool[0].numel(), eng._train_ws.data_ptr(), eng._train_ws.numel()
    first = buffers()
    losses, losses_o, counts = [], [], []
    for i, (SL, TL) in enumerate(lens):
        x, text, t, target = _inputs(cfg, SL, TL, 100 + 3 * i)
        xd, td, tt, tg = x.to(DEV), text.to(DEV), t.to(DEV), target.to(DEV)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        loss = F.mse_loss(m.train_forward_packed(xd, _cu(SL), td, _cu(TL), tt), tg)
        opt.zero_grad(); loss.backward(); opt.step()
        counts.append(torch.cuda.memory_stats()["allocation.all.allocated"] - before)
        losses.append(float(loss))
        assert m.engine(train=True) is eng and buffers() == first, (i, buffers(), first)
        opt_o.zero_grad()
        _, lo, _ = _oracle_packed(cfg, 6, x, text, t, SL, TL, target, sd=sd)
        opt_o.step()
        losses_o.append(lo)
    print("packed loop losses", losses, "oracle", losses_o, "allocations per step", counts)
    assert counts[1] == counts[2] == counts[3], counts          # (step 0 also creates AdamW's state)
    for a, b in zip(losses, losses_o):
        assert abs(a - b) < 3e-2 * b, (losses, losses_o)


def test_tape_records_survive_more_than_64_distinct_tapes():
    """two forwards stay outstanding while > 64 distinct tape addresses pass through the handle: both backwards still find their
    records (they used to be dropped wholesale at the 64th)"""
    cfg = DiTTOConfig(128, 1, 2, 64, 128, 20)
    m = _build(cfg, 1).eval()
    SL, TL = [40, 24], [16, 30]
    x, text, t, target = (z.to(DEV) for z in _inputs(cfg, SL, TL, 5))
    outs = [m.train_forward_packed(x, _cu(SL), text, _cu(TL), t) for _ in range(2)]
    eng = m.engine(train=True)      # (the engine of the parameters' own device: the one the forwards above ran on)
    keep = []
    for i in range(70):   # 70 more forwards, each on a tape of its own (none released)
        o, st = eng.train_forward_packed(x, _cu(SL), text, _cu(TL), t, 0.0, 0)
        keep.append(st)
    assert len({st["tape"].data_ptr() for st in keep}) == 70
    for o in outs:
        m.zero_grad(set_to_none=True)
        F.mse_loss(o, target).backward()
        assert m.proj_out.weight.grad is not None and torch.isfinite(m.proj_out.weight.grad).all()
    for st in keep:
        eng.release_tape_packed(st["tape"])


class _RecSync:
    def __init__(self):
        self.pieces, self.aborts, self.finishes = 0, 0, 0

    def reduce(self, piece):
        self.pieces += 1

    def abort(self):
        self.aborts += 1

    def finish(self):
        self.finishes += 1


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_autograd_refusals_of_both_layouts(layout):
    """The refusals of the training backward, for DiTTO.forward (B = 2, N = 96, T = 40) and DiTTO.train_forward_packed (the same
    rows as lengths [96, 96] / [40, 40]): a second backward through the same output names the method the caller used; a parameter
    changed in place between forward and backward is refused; when the engine's backward raises, the sync's abort() runs once and
    finish() never.
    The engine's backward raises on a grad_output of the wrong shape — a host-side check, nothing is launched.  A loss cannot hand
    one over through backward(): autograd compares every gradient a node returns with the shape of the tensor it belongs to and
    raises itself before this backward runs.  So the node of the output is applied to the wrong-shaped gradient directly
    (out.grad_fn.apply is what autograd calls with the gradient it has accepted)."""
    cfg = DiTTOConfig(256, 3, 4, 64, 256, 20)
    B, N, T, d = 2, 96, 40, 256
    x, text, t, target = (z.to(DEV) for z in _inputs(cfg, [N] * B, [T] * B, 81))
    m = _build(cfg, 5).train()
    if layout == "padded":
        x, text, target = x.view(B, N, d), text.view(B, T, d), target.view(B, N, d)
        who, forward = r"DiTTO\.forward", lambda: m(x, text, t)
    else:
        who, forward = r"DiTTO\.train_forward_packed", lambda: m.train_forward_packed(x, _cu([N] * B), text, _cu([T] * B), t)
    sync = _RecSync()
    m.set_grad_sync(sync, 1)
    out = forward()
    F.mse_loss(out, target).backward()
    assert (sync.pieces, sync.aborts, sync.finishes) == (3, 0, 1)
    with pytest.raises(RuntimeError, match=f"backward through the same {who} twice"):
        F.mse_loss(out, target).backward()
    assert (sync.pieces, sync.aborts, sync.finishes) == (3, 0, 1)            # refused before the engine ran
    # the engine's backward raises: abort() once, no finish(), no piece
    out = forward()
    with pytest.raises(ValueError, match="grad_output"):
        out.grad_fn.apply(torch.ones_like(out)[..., :N // 2, :].contiguous())
    assert (sync.pieces, sync.aborts, sync.finishes) == (3, 1, 1)
    # ... and the same forward's backward still runs afterwards with a sound gradient (its tape was not released)
    F.mse_loss(out, target).backward()
    assert (sync.pieces, sync.aborts, sync.finishes) == (6, 1, 2)
    # a parameter modified in place between forward and backward
    out = forward()
    with torch.no_grad():
        m.proj_in.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="parameters changed between forward and backward"):
        F.mse_loss(out, target).backward()
    assert (sync.pieces, sync.aborts, sync.finishes) == (6, 1, 2)
