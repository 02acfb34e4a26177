"""-m gpu: training a v-predicting network on packed batches — DiTTO.span_noise_packed, train_forward_packed,
span_loss_packed(prediction="v", x0=, t=, loss_weights=), backward().

  * every live parameter gets a finite gradient, and the same step twice gives the same bits;
  * the gradient handed to the prediction's producer is the kernel's grad_pred (engine.span_vloss_packed on the same prediction, with
    the (ca, cs) span_noise_packed derives for t) times grad_output, torch.equal; the loss is the kernel's;
  * halving one utterance's weight halves exactly its rows of that gradient — a power of two, so a bitwise check — and leaves every
    other row's bits alone; context rows are exactly 0;
  * the default prediction="eps" is today's call, bit for bit."""
import pytest
import torch

from ditto_tts_amd.synth import hash_normal
from test_gpu_stream_sampler import SMALL
from test_gpu_train_packed import _build
import vpred_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = SMALL
N, P, Q, TL = (130, 64, 97), (0, 5, 40), (30, 0, 20), (48, 20, 33)
B, D = len(N), CFG.hidden_dim
CU, CU_T = R.cu_of(N), R.cu_of(TL)
T_STEPS = [3, 49, 17]                      # the last timestep included: abar ~ 0 there, where v is the well-conditioned target
WEIGHTS = [1.0, 0.5, 2.0]
TAG = 7


@pytest.fixture(scope="module")
def model():
    return _build(CFG, 4).train()


@pytest.fixture(scope="module")
def data():
    return dict(x0=hash_normal((CU[-1], D), "vpt_x0", 4).to(DEV), text=hash_normal((CU_T[-1], CFG.text_dim), "vpt_text", 4).to(DEV),
                t=torch.tensor(T_STEPS, device=DEV), seeds=torch.tensor([21, 22, 23], dtype=torch.int64, device=DEV))


def _step(m, data, weights, scale=1.0):
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(77)                   # train_forward_packed draws its dropout seed from the CPU generator
    x_in = m.span_noise_packed(data["x0"], CU, list(P), data["t"], seeds=data["seeds"], tag=TAG, suffix_lengths=list(Q))
    pred = m.train_forward_packed(x_in, CU, data["text"], CU_T, data["t"])
    seen = {}
    pred.register_hook(lambda g: seen.setdefault("grad", g.clone()))
    loss = m.span_loss_packed(pred, CU, list(P), seeds=data["seeds"], tag=TAG, suffix_lengths=list(Q), prediction="v", x0=data["x0"],
                              t=data["t"], loss_weights=weights)
    (loss * scale).backward()
    return pred.detach(), loss.detach(), seen["grad"], {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_training_step_hands_the_kernels_gradient_to_the_network(model, data):
    m = model
    pred, loss, g_pred, grads = _step(m, data, WEIGHTS, scale=3.0)
    live = [k for k, _ in m.named_parameters() if ".attn.out_proj." not in k]          # the reference never uses that projection
    assert live and all(k in grads and torch.isfinite(grads[k]).all() for k in live)
    assert all(float(grads[k].abs().max()) > 0 for k in live)
    # the kernel on the same prediction, with the pair span_noise_packed derives for t
    c = m.alphas_cumprod.to(DEV).float()[data["t"].long()]
    want_loss, want_grad = m.engine().span_vloss_packed(pred.float().contiguous(), data["x0"], CU, list(P), c.sqrt().contiguous(),
                                                        (1.0 - c).sqrt().contiguous(), torch.tensor(WEIGHTS, device=DEV),
                                                        seeds=data["seeds"], tag=TAG, suffix_lengths=list(Q))
    assert torch.equal(loss, want_loss) and float(loss) > 0
    assert torch.equal(g_pred, (want_grad * torch.tensor(3.0, device=DEV)).to(pred.dtype))
    gen = R.window_mask(CU, P, Q).to(DEV)
    assert bool((g_pred[~gen] == 0).all()) and bool((g_pred[gen] != 0).any())
    # the same step twice: the same bits
    _, loss2, g2, grads2 = _step(m, data, WEIGHTS, scale=3.0)
    assert torch.equal(loss2, loss) and torch.equal(g2, g_pred) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_halving_a_weight_halves_exactly_that_utterances_rows(model, data):
    m = model
    pred = hash_normal((CU[-1], D), "vpt_pred", 5).to(DEV)
    out = {}
    for name, w in (("full", WEIGHTS), ("half", [WEIGHTS[0], WEIGHTS[1] / 2, WEIGHTS[2]]), ("tensor", torch.tensor(WEIGHTS))):
        p = pred.clone().requires_grad_(True)
        loss = m.span_loss_packed(p, CU, list(P), seeds=data["seeds"], tag=TAG, suffix_lengths=list(Q), prediction="v", x0=data["x0"],
                                  t=data["t"], loss_weights=w)
        loss.backward()
        out[name] = (loss.detach(), p.grad.clone())
    (l_f, g_f), (l_h, g_h), (l_t, g_t) = out["full"], out["half"], out["tensor"]
    assert torch.equal(g_t, g_f) and torch.equal(l_t, l_f)                            # a list and a tensor are the same call
    lo, hi = CU[1], CU[2]
    assert float(g_f[lo:hi].abs().max()) > 0
    assert torch.equal(g_h[lo:hi], g_f[lo:hi] * 0.5)
    assert torch.equal(g_h[:lo], g_f[:lo]) and torch.equal(g_h[hi:], g_f[hi:])
    assert float(l_h) < float(l_f)


def test_default_prediction_is_todays_call(model, data):
    m = model
    pred = hash_normal((CU[-1], D), "vpt_pred", 6).to(DEV)
    kw = dict(seeds=data["seeds"], tag=TAG, suffix_lengths=list(Q))
    want_loss, want_grad = m.engine().span_mse_packed(pred, CU, list(P), **kw)
    for extra in ({}, dict(prediction="eps")):
        p = pred.clone().requires_grad_(True)
        loss = m.span_loss_packed(p, CU, list(P), **kw, **extra)
        loss.backward()
        assert torch.equal(loss.detach(), want_loss) and torch.equal(p.grad, want_grad)
