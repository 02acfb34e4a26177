"""The second-order multistep data-prediction solver, DPM-Solver++(2M) (Lu et al. 2022, alg. 2), restated in float64 from the
paper's form — plain helpers shared by test_multistep_host.py, test_gpu_multistep_update.py and test_gpu_multistep_sampler.py.

With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma), h_i = lambda_{i+1} - lambda_i, r_i = h_{i-1} / h_i:
    x0_i = (x - sigma_i eps) / alpha_i
    D    = x0_i                                                     at step 0
         = (1 + 1 / (2 r_i)) x0_i - (1 / (2 r_i)) x0_{i-1}          with a history
    x'   = (sigma_{i+1} / sigma_i) x - alpha_{i+1} expm1(-h_i) D
and the last step (abar_next = 1, sigma_next = 0) is first order: x' = x0_i.  The timesteps are strided_schedule's."""
import math

import torch


def timesteps(T, n_steps):
    return [int(round(T - 1 - i * (T / n_steps))) for i in range(n_steps)]


class Solver:
    """the solver over the table `alphas_cumprod` (any float dtype; used as float64): step(i, x, eps) -> x', keeping the history"""

    def __init__(self, alphas_cumprod, n_steps):
        ac = alphas_cumprod.double()
        self.taus = timesteps(int(ac.shape[0]), n_steps)
        self.n = n_steps
        self.alpha = [math.sqrt(float(ac[t])) for t in self.taus] + [1.0]
        self.sigma = [math.sqrt(1.0 - float(ac[t])) for t in self.taus] + [0.0]
        self.lam = [math.log(a / s) for a, s in zip(self.alpha[:-1], self.sigma[:-1])]
        self.prev = None

    def step(self, i, x, eps):
        x0 = (x - self.sigma[i] * eps) / self.alpha[i]
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


def update(x, c, u, q, coef, w=None):
    """the kernel's per-element expressions in float64 over fp32 inputs: coef = (a, kx, ke, b, g, use_prev) as the fp32 values the
    kernel is given; u / w None without guidance.  Returns (x', x0, the magnitude the elementwise bound is relative to)."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # noqa: E731
    a, kx, ke, b, g = (f32(v) for v in coef[:5])
    x, c = x.double(), c.double()
    e = c if w is None else f32(w) * (c - u.double()) + u.double()
    x0 = kx * x + ke * e
    hist = g * q.double() if coef[5] else torch.zeros_like(x)
    return a * x + b * x0 + hist, x0, (a * x).abs() + (b * x0).abs() + hist.abs() + 1.0


# ---- the problem with a known answer: data ~ N(0, s2), where the exact eps and the exact ODE solution are closed forms
def gaussian_eps(x, abar, s2):
    """E[eps | x_t = x] for x_0 ~ N(0, s2): sigma_t x / (abar s2 + 1 - abar)"""
    return math.sqrt(1.0 - abar) * x / (abar * s2 + 1.0 - abar)


def gaussian_exact(x_T, abar_T, s2):
    """the probability-flow ODE's solution at abar = 1 from x_T at abar_T: the marginal standard deviations' ratio times x_T"""
    return x_T * math.sqrt(s2) / math.sqrt(abar_T * s2 + 1.0 - abar_T)
