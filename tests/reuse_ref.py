"""Guidance reuse (csrc/guided_reuse.hip) restated in float64 from its definition — plain helpers and the one set of inputs shared by
test_reuse_ref.py (host) and test_gpu_reuse_update.py.  The reference has no guided sampler: like the strided loop, the multistep
solver and the rescale, the feature is pinned by these formulas.

A refresh step keeps delta = fl(c0 - u0), the guidance direction of ITS predictions (one fp32 rounding; delta is an INPUT below, as
the fp32 numbers the kernel reads).  A reuse step (LOAD) then computes, per generated element of utterance b, from this step's
conditional prediction c alone:
    E = c + (w_b - 1) delta
    strided (DDIM):   X' = a_b x + ce_b E + cz_b z
    multistep (2M):   P = kx x + ke E,   X' = a x + b P + (use_prev ? g q : 0),   q' = P

Bound, elementwise, u = 2^-24 the unit roundoff of fp32, A_e = |c| + |(w - 1) delta| (>= |E|):
  * wm1 = fl(w - 1):                        |wm1 - (w - 1)| <= u |w - 1|
  * e = fma(wm1, delta, c), one rounding:   |e - E| <= u |wm1 delta + c| + u |(w - 1) delta| <= u (A_e + |(w - 1) delta|) =: d_e
  strided
  * nz = fl(cz z):                          |nz - cz z| <= u |cz z|
  * i = fma(ce, e, nz):                     |i - I| <= u (|ce| A_e + |cz z|) + |ce| d_e + u |cz z|
  * x' = fma(a, x, i):                      |x' - X'| <= u (|a x| + |ce| A_e + |cz z|) + |i - I|
    in all  u (|a x| + 3 |ce| A_e + |ce (w - 1) delta| + 3 |cz z|)
  multistep
  * m = fl(ke e):                           |m - ke E| <= u |ke| A_e + |ke| d_e
  * p = fma(kx, x, m):                      |p - P| <= u (|kx x| + |ke| A_e) + |m - ke E|
    in all  d_p = u (|kx x| + 3 |ke| A_e + |ke (w - 1) delta|)                      (the bound on q' = p), A_p = |kx x| + |ke| A_e
  * gq = fl(g q):                           |gq - g q| <= u |g q|
  * j = fma(b, p, gq):                      |j - J| <= u (|b| A_p + |g q|) + |b| d_p + u |g q|
  * x' = fma(a, x, j):                      |x' - X'| <= u (|a x| + |b| A_p + |g q|) + |j - J|
    in all  u (|a x| + 2 |b| A_p + 3 |g q|) + |b| d_p
Each is first order in u; SLACK = 1 + 2^-16 covers the dropped second-order terms (a few u relative, 2^-21) and the float64
reference's own roundings (2^-53 relative per operation).  The bound comes from the arithmetic alone, not from anything a kernel
returned.  It is 0 where every term is 0: such an element must be exact."""
import numpy as np
import torch

from ditto_tts_amd.synth import hash_normal

U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -16
STEP = 49                                                            # the scalar Philox tag of every case
# tests/test_gpu_window_update.py's shapes: d, then (rows, prefix rows, suffix rows) per utterance
SHAPES = {"small": (64, ((5, 0, 0), (1, 0, 0), (9, 8, 0), (7, 3, 3), (6, 0, 4), (12, 2, 3))), "stride": (256, ((4202, 1, 1),))}
SEEDS = (5, -6, 2 ** 40 + 7, 8, -(2 ** 33) - 1, 11)
MULTISTEP = dict(a=0.83, kx=1.9, ke=-1.6, b=0.41, g=-0.17)          # one step's row, of the size multistep_schedule gives mid-loop


def cu_of(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


class Inputs:
    """The inputs of one case, on the CPU in fp32: x [S, d], eps2 [2S, d] (a refresh step's [c0; u0]), c [S, d] (a reuse step's
    conditional prediction), q [S, d] (multistep history), z [S, d] (the noise buffer), per-utterance a, ce, cz, w (spread, one
    below 1 and one cz = 0 where there are enough utterances), seeds."""

    def __init__(self, shape):
        self.d, npq = SHAPES[shape]
        self.N, self.P, self.Q = ([v[i] for v in npq] for i in range(3))
        self.B, self.S = len(self.N), sum(self.N)
        B, S, d = self.B, self.S, self.d
        self.cu = cu_of(self.N)
        self.x = hash_normal((S, d), "ru_x", 1)
        self.eps2 = hash_normal((2 * S, d), "ru_eps2", 2)
        self.c = hash_normal((S, d), "ru_c", 3)
        self.q = hash_normal((S, d), "ru_q", 4)
        self.z = hash_normal((S, d), "ru_z", 5)
        k = torch.arange(B, dtype=torch.float32)
        self.a, self.ce = 0.9 + 0.1 * k, -0.2 + 0.15 * k
        self.cz = 0.4 + 0.1 * k
        self.w = 2.0 + 0.75 * k
        if B > 1:
            self.cz[3] = 0.0                                         # a sigma = 0 utterance among noisy ones
            self.w[1] = 0.25                                         # w - 1 < 0
        self.seeds = list(SEEDS[:B])
        self.delta = self.eps2[:S] - self.eps2[S:]                   # fp32: what a refresh step keeps

    def window(self, b):
        return self.cu[b] + self.P[b], self.cu[b + 1] - self.Q[b]

    def gen_mask(self):
        m = torch.zeros(self.S, dtype=torch.bool)
        for b in range(self.B):
            lo, hi = self.window(b)
            m[lo:hi] = True
        return m

    def per_row(self, v):
        """a per-utterance fp32 vector as a float64 column [S, 1]"""
        return torch.cat([torch.full((self.N[b], 1), float(v[b]), dtype=torch.float64) for b in range(self.B)])


def philox_rows(seed, tag, rows, d):
    """ditto_noise_normal's numbers for one utterance of `rows` rows (oracle/philox.py), rounded to fp32"""
    from oracle.philox import noise_normal
    return torch.from_numpy(noise_normal(int(seed), int(tag), rows * d).astype(np.float32)).reshape(rows, d)


def philox_window(inp, global_index=False):
    """[S, d]: every utterance's draw at the WINDOW-local index (0 on the context rows); global_index models the defect of counting
    from the utterance's first row"""
    z = torch.zeros(inp.S, inp.d)
    for b in range(inp.B):
        lo, hi = inp.window(b)
        if global_index:
            z[lo:hi] = philox_rows(inp.seeds[b], STEP, inp.N[b], inp.d)[inp.P[b]:inp.P[b] + hi - lo]
        else:
            z[lo:hi] = philox_rows(inp.seeds[b], STEP, hi - lo, inp.d)
    return z


def _masked(inp, *ts):
    g = inp.gen_mask()[:, None]
    zero = torch.zeros((), dtype=torch.float64)
    return [torch.where(g, torch.nan_to_num(t.double().cpu()), zero) for t in ts]


def load_fp64(inp, c, delta, x, z=None):
    """the strided LOAD step: (x' [S, d], bound [S, d]) in float64, both 0 on the context rows.  z: the noise as the kernel reads or
    draws it ([S, d] fp32), or None (no noise: the cz z term is absent)"""
    c, dl, x = _masked(inp, c, delta, x)
    a, ce, w = inp.per_row(inp.a), inp.per_row(inp.ce), inp.per_row(inp.w)
    czz = torch.zeros_like(x) if z is None else inp.per_row(inp.cz) * _masked(inp, z)[0]
    wd = (w - 1.0) * dl
    out = a * x + ce * (c + wd) + czz
    A_e = c.abs() + wd.abs()
    bound = U32 * SLACK * ((a * x).abs() + 3 * ce.abs() * A_e + (ce * wd).abs() + 3 * czz.abs())
    return out, bound


def multistep_load_fp64(inp, c, delta, x, q, use_prev, k=MULTISTEP):
    """the multistep LOAD step: (x', bound on x', q', bound on q') in float64, 0 on the context rows"""
    c, dl, x, q = _masked(inp, c, delta, x, q)
    f = lambda v: float(np.float32(v))                               # noqa: E731   the fp32 values the kernel is given
    a, kx, ke, b, g = (f(k[n]) for n in ("a", "kx", "ke", "b", "g"))
    w = inp.per_row(inp.w)
    wd = (w - 1.0) * dl
    A_e = c.abs() + wd.abs()
    p = kx * x + ke * (c + wd)
    gq = g * q if use_prev else torch.zeros_like(q)
    out = a * x + b * p + gq
    d_p = U32 * ((kx * x).abs() + 3 * abs(ke) * A_e + (ke * wd).abs())
    A_p = (kx * x).abs() + abs(ke) * A_e
    d_o = U32 * ((a * x).abs() + 2 * abs(b) * A_p + 3 * gq.abs()) + abs(b) * d_p
    return out, SLACK * d_o, p, SLACK * d_p


def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound, with 0 / 0 = 0 and x / 0 = inf (an element that must be exact)"""
    err = (got.double().cpu() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                         torch.zeros_like(err)))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------- fp32 imitation
def _fma(a, b, c):
    """fl32(a b + c) for fp32 arrays: the product is exact in float64 (24 x 24 bits), so adding there and rounding once to fp32
    differs from a true fma only in a double-rounding tie"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _delta_used(inp, bug):
    """delta [S, d] as the (possibly wrong) kernel would read it on each utterance's window rows"""
    dl = inp.delta.numpy().copy()
    if bug == "delta_sign":                                          # u - c kept at the refresh
        dl = (inp.eps2[inp.S:] - inp.eps2[:inp.S]).numpy()
    if bug == "delta_uncond":                                        # taken from the unconditional rows of the refresh's eps
        dl = inp.eps2[inp.S:].numpy().copy()
    if bug == "delta_global":                                        # indexed from the buffer's first row, not the window's
        src, dl = dl, dl.copy()
        for b in range(inp.B):
            lo, hi = inp.window(b)
            dl[lo:hi] = src[:hi - lo]
    return dl


def imitate_load(inp, noise, multistep=False, use_prev=True, bug=None):
    """The LOAD kernels' arithmetic on the host in fp32 (numpy) -> x' [S, d] (strided) or (x', q') (multistep), context rows as in
    the input.  noise: "none", "buffer" or "philox".  `bug` models a wrong kernel: "w_not_wm1" (w in the place of w - 1),
    "delta_sign" (u - c kept), "delta_global" (delta indexed from row 0), "global_philox" (the quad index counted from the utterance's
    first row), "delta_uncond" (delta read from the unconditional rows), "no_kx" (multistep: the kx x term missing)."""
    f = np.float32
    x, c, q = inp.x.numpy().copy(), inp.c.numpy(), inp.q.numpy().copy()
    dl = _delta_used(inp, bug)
    z = None
    if not multistep and noise == "buffer":
        z = inp.z.numpy()
    if not multistep and noise == "philox":
        z = philox_window(inp, global_index=bug == "global_philox").numpy()
    out, qo = x.copy(), q.copy()
    for b in range(inp.B):
        lo, hi = inp.window(b)
        w = f(inp.w[b])
        wm1 = w if bug == "w_not_wm1" else f(w - f(1.0))
        e = _fma(np.full_like(c[lo:hi], wm1), dl[lo:hi], c[lo:hi])
        if multistep:
            k = {n: f(v) for n, v in MULTISTEP.items()}
            m = (k["ke"] * e).astype(f)
            p = m if bug == "no_kx" else _fma(np.full_like(m, k["kx"]), x[lo:hi], m)
            gq = (k["g"] * q[lo:hi]).astype(f) if use_prev else np.zeros_like(m)
            j = _fma(np.full_like(m, k["b"]), p, gq)
            out[lo:hi] = _fma(np.full_like(m, k["a"]), x[lo:hi], j)
            qo[lo:hi] = p
            continue
        nz = np.zeros_like(e) if z is None else (f(inp.cz[b]) * z[lo:hi]).astype(f)
        i = _fma(np.full_like(e, f(inp.ce[b])), e, nz)
        out[lo:hi] = _fma(np.full_like(e, f(inp.a[b])), x[lo:hi], i)
    return (torch.from_numpy(out), torch.from_numpy(qo)) if multistep else torch.from_numpy(out)
