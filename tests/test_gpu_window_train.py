"""-m gpu: span-masked training with the span ANYWHERE (csrc/span_train.hip; DiTTO.span_noise_packed / span_loss_packed with
suffix_lengths=).

Kernel level, both modes (a noise buffer, seeds): x_in is bit-equal to x0 on both contexts and, on the window, torch.equal to the
existing entry run on the window rows compacted into a batch of G_b-row utterances; grad_eps is exactly 0 on both contexts (eps and the
noise hold NaN there) and on the window equals the compacted call's (the same n_elems: no rescaling); the loss is within 1e-5 relative
of a float64 sum, the fp32-output tolerance of tests/test_gpu_span_train.py.  The seeded mode equals the buffer mode fed with
ditto_noise_normal over G_b rows and repeats bit for bit.  With every Q_b = 0, x_in, grad_eps and the loss are torch.equal to the
existing entries' (the same max_N, hence the same partial layout).  End to end: one training step with windows against fp32 autograd
of the oracle per utterance on [prefix; noised; suffix], with the model, tolerances and method of
tests/test_gpu_span_train.py::test_training_step_against_the_oracle_per_utterance, and the same step twice gives the same bits."""
import pytest
import torch

from ditto_tts_amd.synth import hash_normal, synthetic_state_dict
from test_gpu_span_train import _cu
from test_gpu_stream_sampler import SMALL, _model
from test_gpu_train_packed import _build, _check_grads, _oracle_forward_one
from test_gpu_window_update import SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _npq(shape):
    d, npq = SHAPES[shape]
    return (d,) + tuple([v[i] for v in npq] for i in range(3))


def _mask(N, P, Q):
    cu = _cu(N)
    gen = torch.zeros(cu[-1], dtype=torch.bool)
    for b in range(len(N)):
        gen[cu[b] + P[b]:cu[b + 1] - Q[b]] = True
    return cu, gen


def _philox_buffer(eng, N, P, Q, d, seeds, tag):
    """ditto_noise_normal(seeds, tag) over G_b rows per utterance, placed on the window rows of a packed [S, d] buffer (NaN on the
    context rows: they are never read)"""
    cu, _ = _mask(N, P, Q)
    G = [n - p - q for n, p, q in zip(N, P, Q)]
    z = torch.empty(len(N), max(G), d, dtype=torch.float32, device=DEV)
    eng.noise_normal_(z, seeds, tag)
    buf = torch.full((cu[-1], d), float("nan"), dtype=torch.float32, device=DEV)
    for b in range(len(N)):
        buf[cu[b] + P[b]:cu[b + 1] - Q[b]] = z[b, :G[b]]
    return buf


def _seeds(B):
    return torch.tensor([11, -12, 2 ** 41 + 5, 14, -(2 ** 33) - 3, 16][:B], dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def eng():
    m = _model(SMALL)
    e = m.engine(torch.device("cuda:0"))
    e._owner = m                                         # the engine lives with its module
    return e


@pytest.mark.parametrize("mode", ["buffer", "seeded"])
@pytest.mark.parametrize("shape", ["small", "stride"])
def test_window_kernels_against_the_existing_entries_on_the_compacted_rows(eng, shape, mode):
    d, N, P, Q = _npq(shape)
    B = len(N)
    cu, gen = _mask(N, P, Q)
    G = [n - p - q for n, p, q in zip(N, P, Q)]
    S, tag = cu[-1], 0x9E3779B1
    gen_d = gen.to(DEV)
    x0, eps = hash_normal((S, d), "wt_x0", 1).to(DEV), hash_normal((S, d), "wt_eps", 1).to(DEV)
    k = torch.arange(B, dtype=torch.float32)
    ca, cs = (0.95 - 0.1 * k).to(DEV), (0.31 + 0.1 * k).to(DEV)
    seeds = _seeds(B)
    z_full = _philox_buffer(eng, N, P, Q, d, seeds, tag)                 # NaN on the contexts
    eps_in = eps.clone()
    eps_in[~gen_d] = float("nan")                                        # eps is not read on the contexts
    noise_kw = dict(noise=z_full) if mode == "buffer" else dict(seeds=seeds, tag=tag)
    x_in = eng.span_noise_packed(x0, cu, P, ca, cs, suffix_lengths=Q, **noise_kw)
    loss, grad = eng.span_mse_packed(eps_in, cu, P, suffix_lengths=Q, **noise_kw)
    # expected: the existing entries over the window rows alone (P = 0), the same mode
    cg = _cu(G)
    noise_g = dict(noise=z_full[gen_d].contiguous()) if mode == "buffer" else dict(seeds=seeds, tag=tag)
    want_x = eng.span_noise_packed(x0[gen_d].contiguous(), cg, [0] * B, ca, cs, **noise_g)
    want_loss, want_grad = eng.span_mse_packed(eps[gen_d].contiguous(), cg, [0] * B, **noise_g)
    assert torch.isfinite(x_in).all() and torch.isfinite(grad).all() and torch.isfinite(want_x).all()
    assert torch.equal(x_in[~gen_d], x0[~gen_d]), "a context row of x_in is not a bit copy of x0"
    assert torch.equal(x_in[gen_d], want_x)
    assert not torch.equal(x_in[gen_d], x0[gen_d])
    assert torch.all(grad[~gen_d] == 0)
    assert torch.equal(grad[gen_d], want_grad) and float(want_grad.abs().max()) > 0
    # the loss against a float64 sum over the window
    diff = (eps[gen_d].double() - z_full[gen_d].double())
    want64 = float((diff ** 2).sum() / (d * sum(G)))
    print(f"{shape} {mode}: loss {float(loss):.8f} float64 {want64:.8f} rel {abs(float(loss) - want64) / want64:.3e} "
          f"compacted {float(want_loss):.8f}")
    assert abs(float(loss) - want64) <= 1e-5 * want64
    # a repeated call gives the same bits
    loss2, grad2 = eng.span_mse_packed(eps_in, cu, P, suffix_lengths=Q, **noise_kw)
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad)


@pytest.mark.parametrize("shape", ["small", "stride"])
def test_seeded_mode_is_the_buffer_mode_on_noise_normal(eng, shape):
    d, N, P, Q = _npq(shape)
    B = len(N)
    cu, gen = _mask(N, P, Q)
    S, tag = cu[-1], 77
    seeds = _seeds(B)
    x0, eps = hash_normal((S, d), "wt_x0", 2).to(DEV), hash_normal((S, d), "wt_eps", 2).to(DEV)
    ca, cs = torch.full((B,), 0.8, device=DEV), torch.full((B,), 0.6, device=DEV)
    buf = _philox_buffer(eng, N, P, Q, d, seeds, tag)
    x_b = eng.span_noise_packed(x0, cu, P, ca, cs, noise=buf, suffix_lengths=Q)
    x_s = eng.span_noise_packed(x0, cu, P, ca, cs, seeds=seeds, tag=tag, suffix_lengths=Q)
    assert torch.isfinite(x_s).all() and torch.equal(x_s, x_b)
    l_b, g_b = eng.span_mse_packed(eps, cu, P, noise=buf, suffix_lengths=Q)
    l_s, g_s = eng.span_mse_packed(eps, cu, P, seeds=seeds, tag=tag, suffix_lengths=Q)
    l_2, g_2 = eng.span_mse_packed(eps, cu, P, seeds=seeds, tag=tag, suffix_lengths=Q)
    assert torch.equal(g_s, g_b) and torch.equal(l_s, l_b)
    assert torch.equal(g_2, g_s) and torch.equal(l_2, l_s)
    assert float(l_s) > 0


@pytest.mark.parametrize("mode", ["buffer", "seeded"])
@pytest.mark.parametrize("shape", ["small", "stride"])
def test_suffix_lengths_all_zero_is_the_existing_entries(eng, shape, mode):
    d, N, P, _ = _npq(shape)
    B = len(N)
    cu = _cu(N)
    S, tag = cu[-1], 5
    seeds = _seeds(B)
    x0, eps, z = (hash_normal((S, d), "wt_" + k, 3).to(DEV) for k in ("x0", "eps", "z"))
    ca, cs = torch.full((B,), 0.8, device=DEV), torch.full((B,), 0.6, device=DEV)
    kw = dict(noise=z) if mode == "buffer" else dict(seeds=seeds, tag=tag)
    want_x = eng.span_noise_packed(x0, cu, P, ca, cs, **kw)
    want_l, want_g = eng.span_mse_packed(eps, cu, P, **kw)
    got_x = eng.span_noise_packed(x0, cu, P, ca, cs, suffix_lengths=[0] * B, **kw)
    got_l, got_g = eng.span_mse_packed(eps, cu, P, suffix_lengths=[0] * B, **kw)
    assert torch.isfinite(want_x).all() and torch.isfinite(want_g).all()
    assert torch.equal(got_x, want_x) and torch.equal(got_g, want_g) and torch.equal(got_l, want_l)
    got0 = eng.span_noise_packed(x0, cu, None, ca, cs, suffix_lengths=[0] * B, **kw)         # without prompt lengths: P = 0
    assert torch.equal(got0, eng.span_noise_packed(x0, cu, [0] * B, ca, cs, **kw))


def _train_step(m, x0, cu, P, Q, text, cu_t, t, seeds, tag, torch_seed):
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(torch_seed)                       # train_forward_packed draws its dropout seed from the CPU generator
    x_in = m.span_noise_packed(x0, cu, P, t, seeds=seeds, tag=tag, suffix_lengths=Q)
    eps = m.train_forward_packed(x_in, cu, text, cu_t, t)
    loss = m.span_loss_packed(eps, cu, P, seeds=seeds, tag=tag, suffix_lengths=Q)
    loss.backward()
    return x_in, float(loss.detach()), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_training_step_with_windows_against_the_oracle_per_utterance():
    cfg = SMALL
    N, P, Q, TL = (150, 64, 97), (0, 5, 40), (30, 0, 20), (48, 20, 33)
    B, d = len(N), cfg.hidden_dim
    cu, cu_t = _cu(N), _cu(TL)
    _, gen = _mask(N, P, Q)
    x0 = hash_normal((cu[-1], d), "wt_x0", 4)
    text = hash_normal((cu_t[-1], cfg.text_dim), "wt_text", 4)
    t = torch.tensor([3, 31, 17])
    seeds, tag = torch.tensor([21, 22, 23], dtype=torch.int64, device=DEV), 7
    m = _build(cfg, 4).train()
    args = (x0.to(DEV), cu, list(P), list(Q), text.to(DEV), cu_t, t.to(DEV), seeds, tag, 77)
    x_in, loss, grads = _train_step(m, *args)
    _, loss2, grads2 = _train_step(m, *args)
    assert loss2 == loss and all(torch.equal(grads[k], grads2[k]) for k in grads), "the same step twice gave other bits"
    # the oracle: fp32 autograd per utterance on [prefix; noised; suffix] (the kernel's own x_in and z), masked MSE over the batch's n
    z = _philox_buffer(m.engine(), N, P, Q, d, seeds, tag).cpu()
    x_in = x_in.cpu()
    assert torch.equal(x_in[~gen], x0[~gen])
    torch.manual_seed(77)
    drop_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in synthetic_state_dict(cfg, 4).items()}
    n = d * int(gen.sum())
    want_loss = 0.0
    for b in range(B):
        xb, tb = x_in[cu[b]:cu[b + 1]][None], text[cu_t[b]:cu_t[b + 1]][None]
        ob = _oracle_forward_one(sd, cfg, xb, tb, t[b:b + 1], b, B, 0.1, drop_seed, max(N), max(TL))
        lb = ((ob[0, P[b]:N[b] - Q[b]] - z[cu[b] + P[b]:cu[b + 1] - Q[b]]) ** 2).sum() / n
        lb.backward()
        want_loss += float(lb.detach())
    want = {k: v.grad for k, v in sd.items() if v.requires_grad}
    print(f"window training step: loss {loss:.6f} oracle {want_loss:.6f}")
    assert abs(loss - want_loss) < 2e-2 * want_loss
    _check_grads(m, want, 3e-2, "window training step:")
