"""The fused optimizer's chain (ditto_tts_amd/optim.py, csrc/optim.hip) restated in float64 from its definitions — plain helpers shared
by test_optim_ref.py, test_gpu_optim_kernel.py and test_gpu_optim_train.py.  The reference trainer has torch.optim.AdamW and nothing
else (src/TrainDiTTO.py:52): clipping and the EMA are pinned by these formulas, which test_optim_ref.py checks once against torch.

    norm  = sqrt(sum g^2) over every gradient;  clip = min(1, max_norm / (norm + 1e-6))    torch.nn.utils.clip_grad_norm_
    gs = clip g;  pd = p (1 - lr wd)                                                       torch's single-tensor AdamW:
    m' = b1 m + (1 - b1) gs;   v' = b2 v + (1 - b2) gs^2                                   decoupled decay first,
    p' = pd - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),   bc_k = 1 - b_k^t             then the Adam term
    ema' = ema + (1 - decay) (p' - ema)                                                    Tensor.lerp_

Bounds (chain_fp64's second result), elementwise, from the roundings of the expression in the header comment of csrc/optim.hip, to
first order in u = 2^-24, every constant one unit above what the count gives (the dropped second-order terms, the fp64 arithmetic of
the uniform factors, and the 1e-11 of the norm inside clip).  fl(x) of a uniform factor is one rounding, relative u.
  * gs^ = fl(g fl(clip)): two roundings, |gs^ - gs| <= 2u |gs|
  * m'^ = fma(fl(b1), m, fl(fl(1 - b1) gs^)): A = b1 m carries u (its factor), B = (1 - b1) gs carries 1 + 2 + 1 = 4u, the fma one
    rounding of the sum, <= u (|A| + |B|):  |m'^ - m'| <= u (2 |A| + 5 |B|) <= 5u (|A| + |B|);   BOUND_M = 6
  * v'^: gs^2 carries 4u, its rounding 1, the factor 1, the product 1 = 7u on B = (1 - b2) gs^2, u on A = b2 v, u on the sum; all
    terms are >= 0, so |v'^ - v'| <= 8u v';   BOUND_V = 9
  * D^ = fma(sqrtf(v'^), fl(1 / sqrt(bc2)), fl(eps)): the root halves v'^'s 9u and adds one ulp (2u: the compiler's sqrtf is within
    1 ulp), the factor u, the fma u: 8.5u on the first term, 2u on eps, both >= 0:  |D^ - D| <= 9u D
  * q^ = m'^ / D^ (correctly rounded): |q^ - q| <= BOUND_M u (|A| + |B|) / D + 10u |q|
  * p'^ = fma(-fl(lr / bc1), q^, fl(p fl(1 - lr wd))): pd carries 2u, the step size u, the fma u |p'|:
        |p'^ - p'| <= u (|p'| + 3 |pd|) + ss (BOUND_M u (|A| + |B|) / D + 12u |q|),  ss = lr / bc1
  * ema'^ = fma(fl(1 - decay), fl(p'^ - ema), ema):  <= (1 - decay) bound_p + u (3 (1 - decay) |p' - ema| + |ema'|)
The norm: every one of the n squares enters an fp64 fma chain or tree whose partial sums are <= the total, so the sum is within
n 2^-53 relative whatever the order, the root halves that and adds one rounding:  NORM_RTOL(n) = (n + 4) 2^-53 covers the kernel and
a float64 reference summed in any other order.
"""
import math

import numpy as np
import torch

from vpred_ref import worst_ratio  # noqa: F401  (re-exported: the tests use it on these bounds)

U32 = 2.0 ** -24
U64 = 2.0 ** -53
BOUND_M, BOUND_V = 6.0, 9.0
CHUNK = 4096 * 4                      # elements of one chunk (DITTO_OPTIM_CHUNK_QUADS quads)

# the kernel-level case: the smallest sizes that can go wrong — below a quad, a quad, a quad + 1, an odd size of several lanes, exactly
# one chunk, one chunk + 1 (a one-element tail chunk), three chunks + 5 (whole chunks, then a tail with a partial quad)
CASE_SIZES = (1, 3, 4, 5, 1023, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
CASE_GROUPS = ((0.05, 0.5), (0.02, 0.1))          # (lr, weight_decay); segment i belongs to group i % 2
CASE_NO_EMA = 4                                   # this segment keeps no average
CASE_BETAS, CASE_EPS, CASE_DECAY = (0.9, 0.999), 1e-8, 0.99
CASE_MAX_NORM = 10.0                              # the gradients below have a global norm of ~36: clip ~ 0.28
CASE_STEPS = 3


def norm_rtol(n: int) -> float:
    return (n + 4) * U64


def case_params():
    """(p, ema) lists of fp32 CPU tensors: weights of ~0.05, the average somewhere else"""
    gen = torch.Generator().manual_seed(20240601)
    p = [0.05 * torch.randn(n, generator=gen) for n in CASE_SIZES]
    ema = [x + 0.01 * torch.randn(x.shape, generator=gen) for x in p]
    return p, ema


def case_grads(step: int):
    """the gradients of step 1, 2, ...: fp32 CPU tensors of ~0.1, another scale per segment"""
    gen = torch.Generator().manual_seed(777 + step)
    return [0.1 * (1.0 + 0.25 * (i % 3)) * torch.randn(n, generator=gen) for i, n in enumerate(CASE_SIZES)]


def case_lr_wd(i: int):
    return CASE_GROUPS[i % 2]


def global_norm(grads) -> float:
    """sqrt(sum g^2) in float64"""
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


def clip_factor(norm: float, max_norm) -> float:
    """clip_grad_norm_'s coefficient (exactly 1.0 with clipping off)"""
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def chain_fp64(p, g, m, v, ema, step, lr, wd, betas=CASE_BETAS, eps=CASE_EPS, decay=CASE_DECAY, clip=1.0):
    """One tensor's step number `step` (1-based) from fp32 (or float64) inputs, in float64; ema may be None.
    -> ({"p", "m", "v", "ema"}, the elementwise bounds under the same keys)"""
    b1, b2 = betas
    p, g, m, v = (t.double() for t in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    gs = clip * g
    pd = p * (1.0 - lr * wd)
    A, B = b1 * m, (1.0 - b1) * gs
    mn = A + B
    vn = b2 * v + (1.0 - b2) * gs * gs
    D = vn.sqrt() / math.sqrt(bc2) + eps
    q = mn / D
    ss = lr / bc1
    pn = pd - ss * q
    bm = BOUND_M * U32 * (A.abs() + B.abs())
    bp = U32 * (pn.abs() + 3.0 * pd.abs()) + ss * (bm / D + 12.0 * U32 * q.abs())
    out, bound = {"p": pn, "m": mn, "v": vn}, {"p": bp, "m": bm, "v": BOUND_V * U32 * vn}
    if ema is not None:
        e = ema.double()
        en = e + (1.0 - decay) * (pn - e)
        out["ema"] = en
        bound["ema"] = (1.0 - decay) * bp + U32 * (3.0 * (1.0 - decay) * (pn - e).abs() + en.abs())
    return out, bound


# ---------------------------------------------------------------------------------------------------------------- fp32 imitation
F = np.float32


def _fma(a, b, c):
    """fl32(a b + c): the product of two fp32 is exact in float64, so this differs from a true fma only in a double-rounding tie"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


BUGS = ("decay_after", "coupled_l2", "bc2_outside", "clip_on_m", "ema_old_p", "wrong_lr", "tail_dropped")


def imitate(p, g, m, v, ema, step, lr, wd, betas=CASE_BETAS, eps=CASE_EPS, decay=CASE_DECAY, clip=1.0, bug=None):
    """The kernel's arithmetic for one tensor on the host in fp32 (numpy arrays in, a dict of fp32 arrays out).  `bug` models a wrong
    kernel: "decay_after" (the decay applied to p after the Adam term), "coupled_l2" (wd p added to the gradient instead of the
    decoupled decay), "bc2_outside" (sqrt(v') / bc2), "clip_on_m" (the clip factor on m' instead of on g), "ema_old_p" (the average
    taken towards the old p), "tail_dropped" (the elements behind the last whole quad left as they were).  ("wrong_lr" is the
    caller's: it passes another segment's lr and wd.)"""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p0, m0, v0 = (np.asarray(t, F) for t in (p, m, v))
    g = np.asarray(g, F)
    clip32 = F(clip)
    dk = F(1.0 - lr * wd)
    rs2 = F(1.0 / bc2) if bug == "bc2_outside" else F(1.0 / math.sqrt(bc2))
    nss = -F(lr / bc1)
    gs = g if bug == "clip_on_m" else (g * clip32).astype(F)
    if bug == "coupled_l2":
        gs = _fma(F(wd), p0, gs)
        dk = F(1.0)
    pd = p0 if bug == "decay_after" else (p0 * dk).astype(F)
    mn = _fma(F(b1), m0, (F(1.0 - b1) * gs).astype(F))
    if bug == "clip_on_m":
        mn = (mn * clip32).astype(F)
    vn = _fma(F(b2), v0, (F(1.0 - b2) * (gs * gs).astype(F)).astype(F))
    den = _fma(np.sqrt(vn).astype(F), rs2, F(eps))
    pn = _fma(nss, (mn / den).astype(F), pd)
    if bug == "decay_after":
        pn = (pn * dk).astype(F)
    out = {"p": pn, "m": mn, "v": vn}
    if ema is not None:
        e0 = np.asarray(ema, F)
        out["ema"] = _fma(F(1.0 - decay), ((p0 if bug == "ema_old_p" else pn) - e0).astype(F), e0)
    if bug == "tail_dropped" and len(p0) % 4:
        k = len(p0) - len(p0) % 4
        for key, old in (("p", p0), ("m", m0), ("v", v0)) + ((("ema", np.asarray(ema, F)),) if ema is not None else ()):
            out[key][k:] = old[k:]
    return out


def imitate_norm(grads) -> float:
    """the global norm with fp64 sums in an order that is NOT the kernel's: element by element within a tensor (numpy's pairwise sum),
    the tensors last to first"""
    total = 0.0
    for g in reversed(grads):
        total += float(np.sum(np.asarray(g, np.float64) ** 2))
    return math.sqrt(total)
