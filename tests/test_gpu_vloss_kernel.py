"""-m gpu: ditto_span_vloss_window (csrc/span_train.hip), the span loss of a v-predicting network, at kernel level on guarded buffers.

One case (tests/vpred_ref.py CASE_*): d = 64, B = 4, S = 56 from lengths [1, 9, 40, 6]; (P, Q) = (0, 0), (3, 0), (5, 7), (0, 5): no
context, a prompt only, both, a suffix only around a 1-row window; the 40-row utterance spans 3 partials.  Every buffer sits between
guard words; the inputs hold NaN on the context rows (pred, x0, noise), which the kernel must not read.

  * bit-equality: with ca = 1, cs = 0, lw = NULL the gradient, the loss and the workspace partials are torch.equal to
    ditto_span_mse_window's, with a noise buffer and with seeds;
  * against float64 (vpred_ref.vloss_fp64) with spread ca, cs and lw (one of them 0): the gradient elementwise within the DERIVED
    bound (2 lw / n) 7 u (|pred| + |ca z| + |cs x0|), the loss within 1e-5 relative — the bound tests/test_gpu_span_train.py and
    test_gpu_window_train.py hold the MSE kernel's ordered fp32 sum to.  Measured on an MI355X: worst ratio 0.396 (buffer) and 0.396
    (seeded); loss off by 3.3e-10 relative;
  * the gradient is exactly 0 on the context rows, the guards are intact, two calls give the same bits, the seeded mode is the buffer
    mode on ditto_noise_normal's numbers;
  * argument errors: both or neither of noise / seeds, d % 64, a workspace too small; prompt_len and suffix_len both NULL is the whole
    utterance."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal
from gpu_util import stream as _s
from test_gpu_stream_sampler import SMALL, _model
from test_gpu_window_train import _philox_buffer
import vpred_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                             # fp32 words in front of and behind every buffer
MARK = 12345.0
D, N, P, Q = R.CASE_D, list(R.CASE_N), list(R.CASE_P), list(R.CASE_Q)
B, CU = len(N), R.cu_of(R.CASE_N)
S = CU[-1]
N_ELEMS = D * sum(n - p - q for n, p, q in zip(N, P, Q))
N_PART = B * min(1024, (max(N) * D // 4 + 255) // 256)


class Guarded:
    """a contiguous buffer between two runs of GUARD marker words"""

    def __init__(self, t):
        t = t.contiguous()
        self.raw = torch.full((t.numel() + 2 * GUARD,), MARK, dtype=t.dtype, device=DEV)
        self.t = self.raw[GUARD:GUARD + t.numel()].view(t.shape)
        self.t.copy_(t)

    def intact(self):
        return bool((self.raw[:GUARD] == MARK).all() and (self.raw[-GUARD:] == MARK).all())

    @property
    def ptr(self):
        return self.t.data_ptr()


@pytest.fixture(scope="module")
def eng():
    m = _model(SMALL)
    e = m.engine(torch.device("cuda:0"))
    e._owner = m
    return e


@pytest.fixture(scope="module")
def case(eng):
    """the inputs, computed once and left unchanged: pred / x0 with NaN on the context rows, Philox z on the window rows (NaN
    elsewhere), the device lengths, and clean CPU copies for the float64 reference"""
    gen = R.window_mask(CU, P, Q)
    pred, x0 = hash_normal((S, D), "vk_pred", 1), hash_normal((S, D), "vk_x0", 1)
    seeds = torch.tensor(R.CASE_SEEDS, dtype=torch.int64, device=DEV)
    z = _philox_buffer(eng, N, P, Q, D, seeds, R.CASE_TAG)
    nan_ctx = lambda t: torch.where(gen[:, None], t, torch.full((), float("nan")))      # noqa: E731
    i32 = lambda v: Guarded(torch.tensor(v, dtype=torch.int32))                         # noqa: E731
    return dict(gen=gen, pred_cpu=pred, x0_cpu=x0, z_cpu=z.cpu(), pred=Guarded(nan_ctx(pred)), x0=Guarded(nan_ctx(x0)), z=Guarded(z),
                seeds=Guarded(seeds), cu=i32(CU), pl=i32(P), ql=i32(Q))


def _run(case, mode, ca, cs, lw, entry="v", pl=True, ql=True, **over):
    """one call on fresh guarded outputs -> (rc, grad, loss, partials) — the Guarded objects"""
    lib = hip.lib()
    grad, loss, part = Guarded(torch.full((S, D), MARK)), Guarded(torch.full((1,), MARK)), Guarded(torch.full((N_PART,), MARK))
    f32 = lambda v: None if v is None else Guarded(torch.tensor(v, dtype=torch.float32))     # noqa: E731
    cad, csd, lwd = f32(ca), f32(cs), f32(lw)
    noise = case["z"].ptr if mode in ("buffer", "both") else None
    seeds = case["seeds"].ptr if mode in ("seeded", "both") else None
    a = dict(d=D, n=N_ELEMS, wsb=N_PART * 4, pl=case["pl"].ptr if pl else None, ql=case["ql"].ptr if ql else None)
    a.update(over)
    if entry == "v":
        rc = lib.ditto_span_vloss_window(case["pred"].ptr, case["x0"].ptr, noise, seeds, R.CASE_TAG, cad.ptr, csd.ptr,
                                         None if lwd is None else lwd.ptr, case["cu"].ptr, a["pl"], a["ql"], a["n"], grad.ptr, loss.ptr,
                                         part.ptr, a["wsb"], B, S, max(N), a["d"], _s())
    else:
        rc = lib.ditto_span_mse_window(case["pred"].ptr, noise, seeds, R.CASE_TAG, case["cu"].ptr, a["pl"], a["ql"], a["n"], grad.ptr,
                                       loss.ptr, part.ptr, a["wsb"], B, S, max(N), a["d"], _s())
    torch.cuda.synchronize()
    for g in (grad, loss, part, cad, csd, lwd):
        assert g is None or g.intact(), "a guard word was overwritten"
    return rc, grad, loss, part


@pytest.mark.parametrize("mode", ["buffer", "seeded"])
def test_unit_coefficients_give_the_mse_entry_bit_for_bit(case, mode):
    rc_v, g_v, l_v, p_v = _run(case, mode, [1.0] * B, [0.0] * B, None)
    rc_m, g_m, l_m, p_m = _run(case, mode, None, None, None, entry="mse")
    assert rc_v == hip.OK and rc_m == hip.OK
    assert torch.isfinite(g_m.t).all() and float(g_m.t.abs().max()) > 0 and float(l_m.t) > 0
    assert torch.equal(g_v.t, g_m.t) and torch.equal(l_v.t, l_m.t) and torch.equal(p_v.t, p_m.t)
    assert bool((p_v.t != MARK).all())                                   # every partial was written


@pytest.mark.parametrize("mode", ["buffer", "seeded"])
def test_against_float64_within_the_derived_bound(case, mode):
    rc, grad, loss, part = _run(case, mode, R.CASE_CA, R.CASE_CS, R.CASE_LW)
    assert rc == hip.OK
    want_loss, want_grad, bound = R.vloss_fp64(case["pred_cpu"], case["x0_cpu"], case["z_cpu"], R.CASE_CA, R.CASE_CS, R.CASE_LW, CU, P, Q)
    gen = case["gen"]
    g = grad.t.cpu()
    assert torch.isfinite(g).all()
    assert bool((g[~gen] == 0).all()), "the gradient must be exactly 0 on the context rows"
    zero_w = [b for b in range(B) if R.CASE_LW[b] == 0.0]
    assert zero_w and all(bool((g[CU[b]:CU[b + 1]] == 0).all()) for b in zero_w)        # and on an utterance of weight 0
    ratio = R.worst_ratio(g, want_grad, bound)
    rel = abs(float(loss.t) - want_loss) / want_loss
    print(f"{mode}: worst |grad - fp64| / bound {ratio:.3f}; loss {float(loss.t):.8f} fp64 {want_loss:.8f} rel {rel:.2e}")
    assert ratio <= 1.0
    assert rel <= R.LOSS_RTOL
    # the inputs and their guards are as they were
    for k in ("pred", "x0", "z", "seeds", "cu", "pl", "ql"):
        assert case[k].intact(), k
    # a second call gives the same bits
    _, grad2, loss2, part2 = _run(case, mode, R.CASE_CA, R.CASE_CS, R.CASE_LW)
    assert torch.equal(grad2.t, grad.t) and torch.equal(loss2.t, loss.t) and torch.equal(part2.t, part.t)


def test_seeded_mode_is_the_buffer_mode_and_null_weights_are_ones(case):
    _, g_b, l_b, p_b = _run(case, "buffer", R.CASE_CA, R.CASE_CS, R.CASE_LW)
    _, g_s, l_s, p_s = _run(case, "seeded", R.CASE_CA, R.CASE_CS, R.CASE_LW)
    assert torch.equal(g_s.t, g_b.t) and torch.equal(l_s.t, l_b.t) and torch.equal(p_s.t, p_b.t)
    _, g_1, l_1, _ = _run(case, "seeded", R.CASE_CA, R.CASE_CS, [1.0] * B)
    _, g_n, l_n, _ = _run(case, "seeded", R.CASE_CA, R.CASE_CS, None)
    assert torch.equal(g_n.t, g_1.t) and torch.equal(l_n.t, l_1.t)


def test_argument_errors_and_null_lengths(case):
    lib = hip.lib()
    ones, zeros = [1.0] * B, [0.0] * B
    for mode in ("both", "neither"):
        rc, grad, loss, _ = _run(case, mode, ones, zeros, None)
        assert rc == hip.ERR_ARG and b"exactly one" in lib.ditto_last_error()
        assert bool((grad.t == MARK).all()) and float(loss.t) == MARK                  # nothing was launched
    rc, grad, _, _ = _run(case, "seeded", ones, zeros, None, d=96)
    assert rc == hip.ERR_SHAPE and bool((grad.t == MARK).all())
    rc, grad, _, _ = _run(case, "seeded", ones, zeros, None, wsb=N_PART * 4 - 4)
    assert rc == hip.ERR_SIZE and bool((grad.t == MARK).all())
    # prompt_len and suffix_len both NULL: the whole utterance (a clean pred here: every row is read)
    clean = dict(case, pred=Guarded(case["pred_cpu"]), x0=Guarded(case["x0_cpu"]))
    rc, g_null, l_null, p_null = _run(clean, "seeded", R.CASE_CA, R.CASE_CS, R.CASE_LW, pl=False, ql=False, n=S * D)
    zero = dict(clean, pl=Guarded(torch.zeros(B, dtype=torch.int32)), ql=Guarded(torch.zeros(B, dtype=torch.int32)))
    rc0, g_zero, l_zero, p_zero = _run(zero, "seeded", R.CASE_CA, R.CASE_CS, R.CASE_LW, n=S * D)
    assert rc == hip.OK and rc0 == hip.OK and torch.isfinite(g_null.t).all()
    assert torch.equal(g_null.t, g_zero.t) and torch.equal(l_null.t, l_zero.t) and torch.equal(p_null.t, p_zero.t)
    live = [b for b in range(B) if R.CASE_LW[b] != 0.0]
    assert all(bool((g_null.t[CU[b]:CU[b + 1]] != 0).any(dim=1).all()) for b in live)   # every row of a weighted utterance got a gradient
