"""v-prediction (Salimans & Ho 2022; Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.2)
restated in float64 from its definitions — plain helpers shared by test_vpred_host.py, test_gpu_vloss_kernel.py,
test_gpu_vpred_sampler.py and test_gpu_vpred_train.py.  The reference has no v objective and no guided sampler: like the strided
loop, the multistep solver and the rescale, the feature is pinned by these formulas.

With alpha = sqrt(abar), sigma = sqrt(1 - abar) at the step's timestep, the network predicts
    v = alpha z - sigma x0          for x = alpha x0 + sigma z,  so that
    x0 = alpha x - sigma v,   eps = sigma x + alpha v            (alpha^2 + sigma^2 = 1).
Sampling (Strided, Multistep below) recovers (x0, eps) this way and then applies the solver's own definition — DDIM (Song et al.
2021 eq. 12): x' = alpha' x0 + sqrt(1 - abar' - s^2) eps + s z; DPM-Solver++(2M): multistep_ref.Solver on the data prediction.
Nothing here uses the coefficient forms of ditto_tts_amd/sampler.py.

The training loss (ditto_span_vloss_window), per generated element of utterance b, on the fp32 inputs as given:
    target = ca_b z - cs_b x0,  diff = pred - target,  loss = (1 / n) sum lw_b diff^2,  grad = (2 / n) lw_b diff.

Bound on grad (vloss_fp64's third result), u = 2^-24 the unit roundoff of fp32, M = |pred| + |ca z| + |cs x0|:
  * sx = fl(cs x0):                       |sx - cs x0| <= u |cs x0|
  * tg = fl(ca z - sx), one fused rounding: |tg - target| <= u |target| + u |cs x0| <= u (|ca z| + 2 |cs x0|)
  * df = fl(pred - tg):                   |df - diff| <= u |diff| + |tg - target| <= u (M + |ca z| + 2 |cs x0|) <= 3 u M
  * the factor fl(fl(2 / n) lw) and the product with df: three more roundings, each relative u, of a value <= (2 lw / n) M
so |grad^ - grad| <= (2 lw / n) 6 u M to first order; GRAD_ROUNDINGS = 7 leaves one unit for the dropped second-order terms.  The
bound is elementwise and comes from the arithmetic alone, not from anything a kernel returned.
Bound on the loss: the one tests/test_gpu_span_train.py and test_gpu_window_train.py hold the ordered fp32 sum of the MSE kernel to,
|loss^ - loss| <= LOSS_RTOL loss with LOSS_RTOL = 1e-5 (squares are >= 0: no cancellation; the sum is a 256-lane tree over at most
max_N d / 1024 serial adds per lane, then the ordered finish)."""
import math

import numpy as np
import torch

from multistep_ref import Solver, timesteps

U32 = 2.0 ** -24
GRAD_ROUNDINGS = 7
LOSS_RTOL = 1e-5

# the kernel-level case of the host and GPU tests: d, rows per utterance (S = 56), prompt and suffix rows.  Utterance 0: one row, no
# context; 1: a prompt only; 2: both contexts, and 40 rows x 64 columns span 3 partials of 1024 elements; 3: a suffix only, around a
# 1-row window
CASE_D, CASE_N, CASE_P, CASE_Q = 64, (1, 9, 40, 6), (0, 3, 5, 0), (0, 0, 7, 5)
CASE_CA, CASE_CS, CASE_LW = (0.95, 0.6, 0.05, 0.8), (0.31, 0.8, 0.99875, 0.6), (0.0, 0.25, 3.0, 1.0)     # lw = 0 for one utterance
CASE_SEEDS, CASE_TAG = (11, -12, 2 ** 41 + 5, 14), 0x9E3779B1


def cu_of(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


# ---------------------------------------------------------------------------------------------------------------- sampling
class Strided:
    """DDIM over the table `alphas_cumprod` for a v-predicting network: step(i, x, v, z=None) -> x' in float64"""

    def __init__(self, alphas_cumprod, n_steps, eta=0.0):
        ac = alphas_cumprod.double().cpu()
        self.taus = timesteps(int(ac.shape[0]), n_steps)
        self.abar = [float(ac[t]) for t in self.taus] + [1.0]
        self.eta = float(eta)

    def sigma(self, i):
        ab, abp = self.abar[i], self.abar[i + 1]
        return self.eta * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)

    def step(self, i, x, v, z=None):
        ab, abp = self.abar[i], self.abar[i + 1]
        al, sg = math.sqrt(ab), math.sqrt(1 - ab)
        x0, eps = al * x - sg * v, sg * x + al * v
        s = self.sigma(i)
        out = math.sqrt(abp) * x0 + math.sqrt(max(1 - abp - s * s, 0.0)) * eps
        return out if s == 0.0 else out + s * z


class Multistep(Solver):
    """multistep_ref.Solver driven by v: the data prediction is alpha x - sigma v; everything behind it is the solver's own"""

    def step(self, i, x, v):
        x0 = self.alpha[i] * x - self.sigma[i] * v
        if i == self.n - 1:
            out = x0
        else:
            h = self.lam[i + 1] - self.lam[i]
            D = x0
            if i > 0:
                r = (self.lam[i] - self.lam[i - 1]) / h
                D = (1.0 + 0.5 / r) * x0 - (0.5 / r) * self.prev
            out = (self.sigma[i + 1] / self.sigma[i]) * x - self.alpha[i + 1] * math.expm1(-h) * D
        self.prev = x0
        return out


def guided(c, u, w):
    """classifier-free guidance on the network's outputs, whatever they parameterise: u + w (c - u), float64"""
    return u.double() + w * (c.double() - u.double())


# ---------------------------------------------------------------------------------------------------------------- the loss
def window_mask(cu, P, Q):
    gen = torch.zeros(cu[-1], dtype=torch.bool)
    for b in range(len(cu) - 1):
        gen[cu[b] + P[b]:cu[b + 1] - Q[b]] = True
    return gen


def rows_of(cu, P, Q, values):
    """a per-utterance list as a float64 column [S, 1]"""
    return torch.cat([torch.full((cu[b + 1] - cu[b], 1), float(values[b]), dtype=torch.float64) for b in range(len(cu) - 1)])


def vloss_fp64(pred, x0, z, ca, cs, lw, cu, P, Q):
    """(loss, grad [S, d] — 0 on the context rows —, elementwise bound on grad) in float64 from fp32 inputs; ca, cs, lw: the fp32
    values the kernel is given (lw None: 1).  Context rows of pred / x0 / z may hold anything."""
    B = len(cu) - 1
    gen = window_mask(cu, P, Q)
    f32 = lambda vals: [float(torch.tensor(v, dtype=torch.float32)) for v in vals]      # noqa: E731
    a, s = rows_of(cu, P, Q, f32(ca)), rows_of(cu, P, Q, f32(cs))
    w = rows_of(cu, P, Q, f32(lw) if lw is not None else [1.0] * B)
    g2 = gen[:, None]
    zero = torch.zeros((), dtype=torch.float64)
    p, x, n = (torch.where(g2, t.double().cpu(), zero) for t in (pred, x0, z))
    n_el = int(gen.sum()) * pred.shape[1]
    az, sx = a * n, s * x
    diff = torch.where(g2, p - (az - sx), zero)
    loss = float((w * diff * diff).sum() / n_el)
    grad = (2.0 / n_el) * w * diff
    bound = torch.where(g2, (2.0 / n_el) * w * GRAD_ROUNDINGS * U32 * (p.abs() + az.abs() + sx.abs()), zero)
    return loss, grad, bound


def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound, with 0 / 0 = 0 and x / 0 = inf (an element that must be exact)"""
    err = (got.double().cpu() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                         torch.zeros_like(err)))
    return float(r.max())


def philox_rows(seed, tag, rows, d):
    """ditto_noise_normal's numbers for one utterance of `rows` rows (oracle/philox.py, float64 Box-Muller), rounded to fp32"""
    from oracle.philox import noise_normal
    return torch.from_numpy(noise_normal(int(seed), int(tag), rows * d).astype(np.float32)).reshape(rows, d)


def imitate(pred, x0, ca, cs, lw, cu, P, Q, *, z=None, seeds=None, tag=0, bug=None):
    """The kernel's arithmetic on the host in fp32 (numpy): sx = fl(cs x0), tg = fma(ca, z, -sx) — the product is exact in float64
    (24 x 24 bits), so adding there and rounding once to fp32 differs from a true fma only in a double-rounding tie —, df = fl(pred -
    tg), grad = fl(fl(fl(2 / n) lw) df), the loss an fp32 serial sum per utterance times lw (another order than the kernel's: the
    loss bound must admit it).  z: a buffer, or Philox of (seeds[b], tag) at the WINDOW-local index.  -> (loss, grad [S, d]).
    `bug` models a wrong kernel: "cs_sign" (target = ca z + cs x0), "swap" (ca and cs exchanged), "weight_loss_only" (lw on the loss,
    not on the gradient), "global_philox" (the quad index counted from the utterance's first row, not the window's), "suffix_grad"
    (the gradient also written on the suffix rows)."""
    B, d = len(cu) - 1, pred.shape[1]
    f = np.float32
    p32, x32 = pred.cpu().numpy().astype(f), x0.cpu().numpy().astype(f)
    n_el = sum(cu[b + 1] - cu[b] - P[b] - Q[b] for b in range(B)) * d
    scale2 = f(2.0 / n_el)
    grad = np.zeros_like(p32)
    total = f(0.0)
    for b in range(B):
        lo, hi = cu[b] + P[b], cu[b + 1] - Q[b]
        hi_w = cu[b + 1] if bug == "suffix_grad" else hi
        a, s = f(ca[b]), f(cs[b])
        if bug == "swap":
            a, s = s, a
        wt = f(1.0) if lw is None else f(lw[b])
        if z is not None:
            zb = z.cpu().numpy().astype(f)[lo:hi_w]
        elif bug == "global_philox":
            zb = philox_rows(seeds[b], tag, cu[b + 1] - cu[b], d).numpy()[P[b]:P[b] + hi_w - lo]
        else:
            zb = philox_rows(seeds[b], tag, hi_w - lo, d).numpy()
        zb = np.nan_to_num(zb)
        pb, xb = np.nan_to_num(p32[lo:hi_w]), np.nan_to_num(x32[lo:hi_w])
        sx = (s * xb).astype(f)
        if bug == "cs_sign":
            sx = -sx
        tg = (np.float64(a) * zb.astype(np.float64) - sx.astype(np.float64)).astype(f)
        df = (pb - tg).astype(f)
        gs = scale2 if bug == "weight_loss_only" else f(scale2 * wt)
        grad[lo:hi_w] = (gs * df).astype(f)
        acc = f(0.0)
        for row in (df[:hi - lo] * df[:hi - lo]).astype(f):
            acc = f(acc + f(row.sum(dtype=f)))
        total = f(total + f(acc * wt))
    return float(f(total * f(1.0 / n_el))), torch.from_numpy(grad)
