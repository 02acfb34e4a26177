"""-m gpu: the guidance-reuse updates (csrc/guided_reuse.hip) through ditto_guided_update_packed_reuse and
ditto_multistep_update_packed_reuse, on tests/test_gpu_window_update.py's shapes and buffer discipline: guard bands around every
buffer, a sentinel on the context rows of x2, q and delta, NaN on the context rows of eps and of a noise buffer.

STORE (a refresh step) is held to the bits of the EXISTING cfg = 1 window entries on x2 (and q), and delta to torch's fp32 c - u (one
rounding).  LOAD (a reuse step) with every w = 1 is held to the bits of the existing cfg = 0 window entries (e = fma(0, delta, c) = c:
this pins the Philox draw, its window-local index and the coefficient plumbing); with spread w it is held to the float64 reference
and the DERIVED elementwise bound of tests/reuse_ref.py (test_reuse_ref.py shows that bound admitting an fp32 imitation with ratio <=
0.73 and refusing every modelled defect with ratio >= 3e6)."""
import ctypes as C

import pytest
import torch

from ditto_tts_amd import hip
import reuse_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8            # rows in front of and behind every buffer
STORE, LOAD = hip.REUSE_STORE, hip.REUSE_LOAD
NOISES = ["philox", "none", "buffer"]
SHAPE_IDS = ["small", "stride"]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _guarded(t, fill):
    g = torch.full((GUARD, t.shape[1]), fill, dtype=t.dtype, device=DEV)
    pool = torch.cat([g, t, g]).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


def _guards_intact(*pools):
    for pool, fill in pools:
        for band in (pool[:GUARD], pool[-GUARD:]):
            assert torch.isnan(band).all() if fill != fill else torch.all(band == fill)


def _bits(t):
    return t.view(torch.int32)


class Case:
    """reuse_ref.Inputs on the device, with the sentinel / NaN patterns on the context rows"""

    def __init__(self, shape, noise="none", w_one=False):
        self.inp = inp = R.Inputs(shape)
        self.noise, self.d, self.B, self.S, self.N, self.P, self.Q = noise, inp.d, inp.B, inp.S, inp.N, inp.P, inp.Q
        if w_one:
            inp.w[:] = 1.0
        S, d = self.S, self.d
        gen = inp.gen_mask()
        self.gen, self.ctx = torch.nonzero(gen).reshape(-1).to(DEV), torch.nonzero(~gen).reshape(-1).to(DEV)
        self.sent = (torch.arange(len(self.ctx) * d, dtype=torch.float32, device=DEV).reshape(-1, d) % 97) + 1000.0
        self.a, self.ce, self.cz, self.w = (v.to(DEV) for v in (inp.a, inp.ce, inp.cz, inp.w))
        self.seeds = torch.tensor(inp.seeds, dtype=torch.int64, device=DEV) if noise == "philox" else None
        self.cu, self.pl, self.ql = _i32(inp.cu), _i32(inp.P), _i32(inp.Q)
        x = inp.x.to(DEV)
        x[self.ctx] = self.sent
        self.x1 = x                                                  # [S, d]
        self.x2 = torch.cat([x, x])                                  # [2S, d]: [x; x]
        self.eps2 = inp.eps2.to(DEV)                                 # a refresh step's [c0; u0]
        self.delta = (self.eps2[:S] - self.eps2[S:]).contiguous()    # torch, fp32: one rounding
        for h in range(2):
            self.eps2[self.ctx + h * S] = float("nan")
        self.c = inp.c.to(DEV)
        self.c[self.ctx] = float("nan")
        self.q = inp.q.to(DEV)
        self.q[self.ctx] = self.sent + 500.0
        self.z = None
        if noise == "buffer":
            self.z = inp.z.to(DEV)
            self.z[self.ctx] = float("nan")
        self.coef = {use_prev: hip.MultistepCoef(*(R.MULTISTEP[n] for n in ("a", "kx", "ke", "b", "g")), 123.0, use_prev, 0)
                     for use_prev in (0, 1)}                         # its w is ignored

    def delta_in(self, filled):
        """the delta buffer: the kept direction on the window rows (a reuse step) or junk there (a refresh), a sentinel elsewhere"""
        dl = self.delta.clone() if filled else torch.full_like(self.delta, -3.0)
        dl[self.ctx] = self.sent + 250.0
        return dl

    def ctx_args(self, null_ctx=False):
        return (None, None) if null_ctx else (self.pl.data_ptr(), self.ql.data_ptr())

    def reuse(self, x_t, eps_t, delta_t, mode, mirror=0, z=None, null_ctx=False, **over):
        """ditto_guided_update_packed_reuse -> its return code; `over` replaces arguments by name (pointers as ints or None)"""
        a = dict(x=x_t.data_ptr(), eps=eps_t.data_ptr(), delta=delta_t.data_ptr(), z=_ptr(z), seeds=_ptr(self.seeds), step=R.STEP,
                 w=self.w.data_ptr(), a=self.a.data_ptr(), ce=self.ce.data_ptr(), cz=self.cz.data_ptr(), cu=self.cu.data_ptr(),
                 pl=self.ctx_args(null_ctx)[0], ql=self.ctx_args(null_ctx)[1], B=self.B, S=self.S, max_N=max(self.N), d=self.d,
                 mode=mode, mirror=mirror, stream=_s())
        a.update(over)
        return hip.lib().ditto_guided_update_packed_reuse(*a.values())

    def reuse_ms(self, x_t, eps_t, q_t, delta_t, use_prev, mode, mirror=0, null_ctx=False, **over):
        a = dict(x=x_t.data_ptr(), eps=eps_t.data_ptr(), q=q_t.data_ptr(), delta=delta_t.data_ptr(), step=C.byref(self.coef[use_prev]),
                 w=self.w.data_ptr(), cu=self.cu.data_ptr(), pl=self.ctx_args(null_ctx)[0], ql=self.ctx_args(null_ctx)[1], B=self.B,
                 S=self.S, max_N=max(self.N), d=self.d, mode=mode, mirror=mirror, stream=_s())
        a.update(over)
        return hip.lib().ditto_multistep_update_packed_reuse(*a.values())

    def window(self, x, eps, z, cfg):
        """the existing strided window entry, in place on x"""
        hip.check(hip.lib().ditto_guided_update_packed_window(
            x.data_ptr(), eps.data_ptr(), _ptr(z), _ptr(self.seeds), R.STEP, self.w.data_ptr() if cfg else None, self.a.data_ptr(),
            self.ce.data_ptr(), self.cz.data_ptr(), self.cu.data_ptr(), self.pl.data_ptr(), self.ql.data_ptr(), self.B, self.S,
            max(self.N), self.d, cfg, _s()))

    def window_ms(self, x, eps, q, use_prev, cfg):
        hip.check(hip.lib().ditto_multistep_update_window(
            x.data_ptr(), eps.data_ptr(), q.data_ptr(), C.byref(self.coef[use_prev]), None, self.w.data_ptr() if cfg else None,
            self.cu.data_ptr(), self.pl.data_ptr(), self.ql.data_ptr(), self.B, self.S, max(self.N), self.d, cfg, _s()))

    def drawn(self):
        """[S, d]: ditto_noise_normal's bits at the window-local index of every utterance (0 on the context rows)"""
        G = [n - p - q for n, p, q in zip(self.N, self.P, self.Q)]
        out = torch.empty(self.B, max(G) * self.d, dtype=torch.float32, device=DEV)
        hip.check(hip.lib().ditto_noise_normal(out.data_ptr(), self.seeds.data_ptr(), R.STEP, self.B, max(G) * self.d, _s()))
        z = torch.zeros(self.S, self.d, device=DEV)
        for b in range(self.B):
            lo, hi = self.inp.window(b)
            z[lo:hi] = out[b, :G[b] * self.d].reshape(G[b], self.d)
        return z


# ---------------------------------------------------------------------------------------------------------------- STORE
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_store_is_the_cfg_window_update_and_keeps_the_direction(shape, noise):
    c = Case(shape, noise)
    S = c.S
    want = c.x2.clone()
    c.window(want, c.eps2, c.z, 1)
    x_pool, x = _guarded(c.x2, 7.0)
    e_pool, eps = _guarded(c.eps2, float("nan"))
    d_pool, delta = _guarded(c.delta_in(False), 9.0)
    z_pool, z = (None, None) if c.z is None else _guarded(c.z, float("nan"))
    e_before = e_pool.clone()
    hip.check(c.reuse(x, eps, delta, STORE, z=z))
    assert torch.isfinite(want[c.gen]).all()
    assert torch.equal(x, want) and not torch.equal(x[c.gen], c.x2[c.gen])
    assert torch.equal(x[:S], x[S:])
    assert torch.equal(delta[c.gen], c.delta[c.gen])
    assert torch.equal(delta[c.ctx], c.sent + 250.0), "a context row of delta was written"
    for h in range(2):
        assert torch.equal(x[c.ctx + h * S], c.sent), "a context row of x2 was written"
    _guards_intact((x_pool, 7.0), (e_pool, float("nan")), (d_pool, 9.0), *(() if z_pool is None else ((z_pool, float("nan")),)))
    assert torch.equal(_bits(e_pool), _bits(e_before)), "eps was written"


@pytest.mark.parametrize("use_prev", [0, 1])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_multistep_store_is_the_cfg_window_update_and_keeps_the_direction(shape, use_prev):
    c = Case(shape)
    S = c.S
    want, want_q = c.x2.clone(), c.q.clone()
    c.window_ms(want, c.eps2, want_q, use_prev, 1)
    x_pool, x = _guarded(c.x2, 7.0)
    e_pool, eps = _guarded(c.eps2, float("nan"))
    q_pool, q = _guarded(c.q, 5.0)
    d_pool, delta = _guarded(c.delta_in(False), 9.0)
    hip.check(c.reuse_ms(x, eps, q, delta, use_prev, STORE))
    assert torch.isfinite(want[c.gen]).all() and torch.isfinite(want_q[c.gen]).all()
    assert torch.equal(x, want) and torch.equal(q, want_q) and not torch.equal(q[c.gen], c.q[c.gen])
    assert torch.equal(delta[c.gen], c.delta[c.gen]) and torch.equal(delta[c.ctx], c.sent + 250.0)
    assert torch.equal(q[c.ctx], c.sent + 500.0)
    for h in range(2):
        assert torch.equal(x[c.ctx + h * S], c.sent)
    _guards_intact((x_pool, 7.0), (e_pool, float("nan")), (q_pool, 5.0), (d_pool, 9.0))


# ---------------------------------------------------------------------------------------------------------------- LOAD, w = 1
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_load_with_unit_scales_is_the_unguided_window_update(shape, noise):
    c = Case(shape, noise, w_one=True)
    want = c.x1.clone()
    c.window(want, c.c, c.z, 0)
    x = c.x2.clone()
    delta = c.delta_in(True)
    hip.check(c.reuse(x, c.c, delta, LOAD, z=c.z))
    assert torch.isfinite(want[c.gen]).all()
    assert torch.equal(x[:c.S], want) and torch.equal(x[c.S:], c.x2[c.S:])


@pytest.mark.parametrize("use_prev", [0, 1])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_multistep_load_with_unit_scales_is_the_unguided_window_update(shape, use_prev):
    c = Case(shape, w_one=True)
    want, want_q = c.x1.clone(), c.q.clone()
    c.window_ms(want, c.c, want_q, use_prev, 0)
    x, q = c.x2.clone(), c.q.clone()
    hip.check(c.reuse_ms(x, c.c, q, c.delta_in(True), use_prev, LOAD))
    assert torch.isfinite(want[c.gen]).all()
    assert torch.equal(x[:c.S], want) and torch.equal(q, want_q) and torch.equal(x[c.S:], c.x2[c.S:])


# ---------------------------------------------------------------------------------------------------------------- LOAD, spread w
def _on_window(c, t):
    return torch.where(c.inp.gen_mask()[:, None], t.cpu(), torch.zeros(()))


@pytest.mark.parametrize("mirror", [0, 1])
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_load_is_within_the_derived_bound_of_the_fp64_reference(shape, noise, mirror):
    c = Case(shape, noise)
    S = c.S
    zr = None if noise == "none" else c.z if noise == "buffer" else c.drawn()
    want, bound = R.load_fp64(c.inp, c.c, c.delta, c.x1, zr)
    x_pool, x = _guarded(c.x2, 7.0)
    e_pool, eps = _guarded(c.c, float("nan"))                        # exactly [S, d] between its guards
    d_pool, delta = _guarded(c.delta_in(True), 9.0)
    z_pool, z = (None, None) if c.z is None else _guarded(c.z, float("nan"))
    d_before, e_before = d_pool.clone(), e_pool.clone()
    hip.check(c.reuse(x, eps, delta, LOAD, mirror=mirror, z=z))
    ratio = R.worst_ratio(_on_window(c, x[:S]), want, bound)
    print(f"strided load {shape} {noise} mirror {mirror}: worst ratio {ratio:.3f}")
    assert torch.isfinite(x[c.gen]).all() and ratio <= 1.0
    assert not torch.equal(x[c.gen], c.x2[c.gen])
    assert torch.equal(x[c.ctx], c.sent) and torch.equal(x[c.ctx + S], c.sent)
    assert torch.equal(x[S:], x[:S] if mirror else c.x2[S:])
    assert torch.equal(_bits(d_pool), _bits(d_before)), "delta was written"
    assert torch.equal(_bits(e_pool), _bits(e_before)), "eps was written"
    _guards_intact((x_pool, 7.0), *(() if z_pool is None else ((z_pool, float("nan")),)))


@pytest.mark.parametrize("mirror", [0, 1])
@pytest.mark.parametrize("use_prev", [0, 1])
@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_multistep_load_is_within_the_derived_bound_of_the_fp64_reference(shape, use_prev, mirror):
    c = Case(shape)
    S = c.S
    want, bound, want_q, bound_q = R.multistep_load_fp64(c.inp, c.c, c.delta, c.x1, c.q, bool(use_prev))
    x_pool, x = _guarded(c.x2, 7.0)
    e_pool, eps = _guarded(c.c, float("nan"))
    q_pool, q = _guarded(c.q, 5.0)
    d_pool, delta = _guarded(c.delta_in(True), 9.0)
    d_before, e_before = d_pool.clone(), e_pool.clone()
    hip.check(c.reuse_ms(x, eps, q, delta, use_prev, LOAD, mirror=mirror))
    r_x, r_q = R.worst_ratio(_on_window(c, x[:S]), want, bound), R.worst_ratio(_on_window(c, q), want_q, bound_q)
    print(f"multistep load {shape} use_prev {use_prev} mirror {mirror}: worst ratio x' {r_x:.3f}, q' {r_q:.3f}")
    assert torch.isfinite(x[c.gen]).all() and r_x <= 1.0 and r_q <= 1.0
    assert torch.equal(x[c.ctx], c.sent) and torch.equal(x[c.ctx + S], c.sent) and torch.equal(q[c.ctx], c.sent + 500.0)
    assert torch.equal(x[S:], x[:S] if mirror else c.x2[S:])
    assert torch.equal(_bits(d_pool), _bits(d_before)) and torch.equal(_bits(e_pool), _bits(e_before))
    _guards_intact((x_pool, 7.0), (q_pool, 5.0))


# ---------------------------------------------------------------------------------------------------------------- spans, repeats
@pytest.mark.parametrize("mode", [STORE, LOAD], ids=["store", "load"])
def test_null_length_pointers_are_zero_lengths_and_a_repeat_gives_the_same_bits(mode):
    c = Case("small", "philox")
    c.pl, c.ql = _i32([0] * c.B), _i32([0] * c.B)
    eps = c.eps2.nan_to_num(0.5) if mode == STORE else c.c.nan_to_num(0.5)      # no context: every row is read
    outs = []
    for null_ctx in (False, True, True):
        x, delta = c.x2.clone(), c.delta.clone()
        hip.check(c.reuse(x, eps, delta, mode, mirror=int(mode == LOAD), null_ctx=null_ctx))
        xm, q, dm = c.x2.clone(), c.q.clone(), c.delta.clone()
        hip.check(c.reuse_ms(xm, eps, q, dm, 1, mode, mirror=int(mode == LOAD), null_ctx=null_ctx))
        outs.append((x, delta, xm, q, dm))
    assert all(torch.isfinite(t).all() for t in outs[0])
    assert not torch.equal(outs[0][0], c.x2) and not torch.equal(outs[0][2], c.x2)
    for other in outs[1:]:
        for got, want in zip(other, outs[0]):
            assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    c = Case("small", "buffer")
    lib = hip.lib()
    x, q, delta = c.x2.clone(), c.q.clone(), c.delta_in(True)
    S = c.S
    bad = [(dict(delta=None), hip.ERR_ARG, b"delta"), (dict(mode=0), hip.ERR_ARG, b"mode"), (dict(mode=3), hip.ERR_ARG, b"mode"),
           (dict(mode=STORE, mirror=1), hip.ERR_ARG, b"mirror"), (dict(w=None), hip.ERR_ARG, b"w"), (dict(cu=None), hip.ERR_ARG, b"cu"),
           (dict(x=None), hip.ERR_ARG, b"null"), (dict(eps=None), hip.ERR_ARG, b"null"), (dict(d=96), hip.ERR_SHAPE, b"d % 64"),
           (dict(d=0), hip.ERR_SHAPE, b"positive"), (dict(B=0), hip.ERR_SHAPE, b"positive"), (dict(S=0), hip.ERR_SHAPE, b"positive"),
           (dict(max_N=0), hip.ERR_SHAPE, b"positive"), (dict(max_N=S + 1), hip.ERR_SHAPE, b"max_N <= S"),
           (dict(B=65536, S=70000, max_N=2), hip.ERR_SHAPE, b"65535")]
    for over, code, word in bad:
        for mode in (STORE, LOAD):
            kw = {"mode": mode, **over}
            eps = c.eps2 if kw["mode"] == STORE else c.c
            assert c.reuse(x, eps, delta, z=c.z, **kw) == code, (over, mode)
            assert word in lib.ditto_last_error(), (over, lib.ditto_last_error())
            assert c.reuse_ms(x, eps, q, delta, 1, **kw) == code, (over, mode)
            assert word in lib.ditto_last_error(), (over, lib.ditto_last_error())
    assert c.reuse(x, c.c, delta, LOAD, z=c.z, seeds=c.a.data_ptr()) == hip.ERR_ARG and b"exclusive" in lib.ditto_last_error()
    assert c.reuse(x, c.c, delta, LOAD, z=c.z, cz=None) == hip.ERR_ARG
    assert c.reuse_ms(x, c.c, q, delta, 1, LOAD, step=None) == hip.ERR_ARG and b"step" in lib.ditto_last_error()
    assert c.reuse_ms(x, c.c, q, delta, 1, LOAD, q=None) == hip.ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(x, c.x2) and torch.equal(q, c.q) and torch.equal(_bits(delta), _bits(c.delta_in(True)))
