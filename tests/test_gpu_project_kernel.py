"""-m gpu: projected guidance (csrc/guided_project.hip) through the C entries of include/ditto_project.h, on tests/project_ref.py's inputs:
B = 4 utterances at d = 64 (windows of 1 row, 256 rows — exactly one chunk —, 257 and 3 rows), d = 768 (22 rows — a chunk boundary inside a
row —, 70 rows — several chunks —, 1 and 43 rows) and d = 256 with prompts and suffixes; both coefficient pairs, the threshold off, on and
inactive, on and active, beta 0 and -0.5, use_prev 0 with a NaN-filled direction.  Every buffer stands between NaN guard bands and
holds NaN in every row the contract says is not read: the context rows of x2, eps2, the direction, q and a noise buffer, and in the
update launch the whole unconditional half of eps2.

Held: the coefficients inside the DERIVED bounds of project_ref against fp64; the stored direction bit-equal to the restated fp32
chain; x' (and q) bit-equal, in both halves, to the restated fp32 e — from the kernel's own coefficients — sent through the EXISTING
unguided window entries (so the solver lines, the noise and the Philox index are the plain entries' by bits); that e inside its
elementwise bound, the plain-CFG utterances among them; the orthogonality property at eta = 0; everything outside the windows
untouched, bit for bit; the same bits for an utterance at another position, in another B, with max_N exact, over- or under-reported
(another grid: one column strides over all chunks); out-of-range prompt and suffix lengths behave as their clamped values; refused
calls touch nothing."""
import functools

import numpy as np
import pytest
import torch

import project_ref as R
from ditto_tts_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, GUARD_BYTES, FILL = 4, 512, 0xA5
NAN = float("nan")
STEP = 977
MS = dict(a=0.83, kx=R.KX_EPS, ke=R.KE_EPS, b=0.41, g=-0.13)       # a 2M step's host coefficients (its w is not used)
LINES = ["philox", "buffer", "none", "tags", "ms0", "ms1", "ms_coefs"]


def _s():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(t):
    """(pool with NaN guard rows in front and behind, the view the library gets)"""
    g = torch.full((GUARD, t.shape[1]), NAN)
    pool = torch.cat([g, t, g]).to(DEV).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


class Batch:
    """utterances [(shape name, b)] of project_ref packed in the given order; `clean`: no NaN on the context rows (the clamp test)"""

    def __init__(self, utts, clean=False, lens=None):
        self.utts, self.B = list(utts), len(utts)
        self.ids = [b for _, b in utts]
        self.d = R.SHAPES[utts[0][0]][0]
        self.gpq = [R.SHAPES[n][1][b] for n, b in utts] if lens is None else lens
        self.n = [g + p + q for g, p, q in self.gpq]
        self.cu = [0]
        for n in self.n:
            self.cu.append(self.cu[-1] + n)
        self.S, self.max_N = self.cu[-1], max(self.n)
        self.par = [R.case_par(n, b) for n, b in utts]
        S, d = self.S, self.d
        x2, eps2, m = torch.full((2 * S, d), NAN), torch.full((2 * S, d), NAN), torch.full((S, d), NAN)
        self.win = []                                           # per utterance: the window's rows in the packed batch
        for k, (name, b) in enumerate(utts):
            g, p, q = self.gpq[k]
            lo = self.cu[k] + (0 if clean else p)
            hi = self.cu[k + 1] - (0 if clean else q)
            src = slice(0, self.n[k]) if clean else slice(p, p + g)
            x, c, u, mm = (torch.from_numpy(v[src].copy()) for v in R.rows(name, b))
            x2[lo:hi], eps2[lo:hi], eps2[S + lo:S + hi], m[lo:hi] = x, c, u, mm
            self.win.append((self.cu[k] + p, self.cu[k] + p + g))
        self.x2_0, self.eps2_0, self.m_0 = x2, eps2, m
        self.proj = torch.zeros(self.B, 8)
        for k, p_ in enumerate(self.par):
            self.proj[k, :6] = torch.tensor([p_[f] for f in R.PAR_FIELDS[:6]])
            self.proj.view(torch.int32)[k, 6] = p_["use_prev"]
        gen = torch.zeros(S, dtype=torch.bool)
        for lo, hi in self.win:
            gen[lo:hi] = True
        self.gen = gen

    def window_np(self, k):
        """(x, c, u, m) of utterance k's window as the buffers hold them"""
        lo, hi = self.win[k]
        S = self.S
        return tuple(v.numpy() for v in (self.x2_0[lo:hi], self.eps2_0[lo:hi], self.eps2_0[S + lo:S + hi], self.m_0[lo:hi]))

    def device(self, max_N=None):
        """the buffers on the device; the scratch is sized for the max_N the entries will be given (at least the true one)"""
        dv = dict(proj=self.proj.to(DEV), cu=_i32(self.cu), pl=_i32([p for _, p, _ in self.gpq]), ql=_i32([q for _, _, q in self.gpq]))
        for name, t in (("x2", self.x2_0), ("eps2", self.eps2_0), ("m", self.m_0)):
            dv[name + "_pool"], dv[name] = _guarded(t)
        need = hip.lib().ditto_guidance_project_bytes(self.B, max(self.max_N, max_N or 0), self.d)
        assert need > 0
        dv["need"] = need
        dv["spool"] = torch.full((need + 2 * GUARD_BYTES,), FILL, dtype=torch.uint8, device=DEV)
        dv["scratch"] = dv["spool"][GUARD_BYTES:GUARD_BYTES + need]
        assert dv["scratch"].data_ptr() % 256 == 0
        return dv


def project(bt, dv, max_N=None, pl=None, ql=None, **over):
    """launch 1 and the finish -> the status"""
    a = dict(x2=dv["x2"].data_ptr(), eps2=dv["eps2"].data_ptr(), dir=dv["m"].data_ptr(), proj=dv["proj"].data_ptr(),
             cu=dv["cu"].data_ptr(), prompt_len=_ptr(dv["pl"] if pl is None else pl), suffix_len=_ptr(dv["ql"] if ql is None else ql),
             B=bt.B, S=bt.S, max_N=bt.max_N if max_N is None else max_N, d=bt.d, scratch=dv["scratch"].data_ptr(),
             scratch_bytes=dv["need"], stream=_s())
    a.update(over)
    return hip.call("ditto_guidance_project_packed", **a)


def pcoef(bt, dv):
    torch.cuda.synchronize()
    return dv["scratch"][:16 * bt.B].view(torch.float32).view(bt.B, 4).cpu().numpy()


def line_args(bt, line):
    """the solver's own arguments of an update `line`, shared by the project entry and the existing window entry it is held to;
    the per-utterance ones follow the utterance (its id in project_ref), not its slot"""
    B, S, d = bt.B, bt.S, bt.d
    per = lambda table, dtype=torch.float32: torch.tensor([table[b] for b in bt.ids], dtype=dtype, device=DEV)
    la = dict(a=per([0.9, 0.8, 1.1, 0.7]), ce=per([-0.3, 0.2, -0.25, 0.4]), cz=per([0.5, 0.0, 0.3, 0.2]), seeds=None, z=None, tags=None,
              q=None, coef=None, coefs=None)
    if line in ("philox", "tags"):
        la["seeds"] = per([11, 12, 13, 14], torch.int64)
    if line == "tags":
        la["tags"] = per([5, 6, 7, 8], torch.int32)
    if line == "buffer":
        from ditto_tts_amd.synth import hash_normal
        z = hash_normal((S, d), "pj_z", S)
        z[~bt.gen] = NAN
        la["z_pool"], la["z"] = _guarded(z)
    if line.startswith("ms"):
        from ditto_tts_amd.synth import hash_normal
        q = torch.full((S, d), NAN)
        for (lo, hi), b in zip(bt.win, bt.ids):                  # the history follows the utterance
            q[lo:hi] = hash_normal((hi - lo, d), "pj_q", 10 * d + b)
        la["q_pool"], la["q"] = _guarded(q)
        la["coef"] = hip.MultistepCoef(MS["a"], MS["kx"], MS["ke"], MS["b"], MS["g"], 123.0, int(line == "ms1"), 0)
        if line == "ms_coefs":                                   # one ditto_multistep_coef per utterance, use_prev alternating
            co = torch.zeros(B, 8)
            for k, b in enumerate(bt.ids):
                co[k, :6] = torch.tensor([MS["a"] + 0.01 * b, MS["kx"], MS["ke"], MS["b"] - 0.02 * b, MS["g"], 55.0])
                co.view(torch.int32)[k, 6] = b % 2
            la["coefs"], la["coef"] = co.to(DEV), None
    return la


def update(bt, dv, la, x2, eps2, pc, max_N=None, pl=None, ql=None, **over):
    """launch 2 through its entry, in place on x2 (and la's q) -> the status"""
    common = dict(cu=dv["cu"].data_ptr(), prompt_len=_ptr(dv["pl"] if pl is None else pl), suffix_len=_ptr(dv["ql"] if ql is None else ql),
                  B=bt.B, S=bt.S, max_N=bt.max_N if max_N is None else max_N, d=bt.d, stream=_s())
    if la["q"] is None:
        a = dict(x2=x2.data_ptr(), eps2=eps2.data_ptr(), dir=dv["m"].data_ptr(), pcoef=pc.data_ptr(), noise=_ptr(la["z"]),
                 seeds=_ptr(la["seeds"]), step=STEP, tags=_ptr(la["tags"]), a=la["a"].data_ptr(), ce=la["ce"].data_ptr(),
                 cz=la["cz"].data_ptr(), **common)
        a.update(over)
        return hip.call("ditto_guided_update_packed_project", **a)
    a = dict(x2=x2.data_ptr(), eps2=eps2.data_ptr(), q=la["q"].data_ptr(), dir=dv["m"].data_ptr(), pcoef=pc.data_ptr(), step=la["coef"],
             coefs=_ptr(la["coefs"]), **common)
    a.update(over)
    return hip.call("ditto_multistep_update_packed_project", **a)


def existing(bt, dv, la, x, e, q):
    """the EXISTING unguided window entry of the same line on eps = e [S, d], in place on x [S, d] (and q)"""
    lib, sizes = hip.lib(), (bt.B, bt.S, bt.max_N, bt.d, 0, _s())
    ctx = (dv["cu"].data_ptr(), dv["pl"].data_ptr(), dv["ql"].data_ptr())
    if q is not None:
        hip.check(lib.ditto_multistep_update_window(x.data_ptr(), e.data_ptr(), q.data_ptr(), la["coef"], _ptr(la["coefs"]), None, *ctx,
                                                    *sizes))
    elif la["tags"] is not None:
        hip.check(lib.ditto_guided_update_packed_tags_window(x.data_ptr(), e.data_ptr(), _ptr(la["z"]), _ptr(la["seeds"]),
                                                             la["tags"].data_ptr(), None, la["a"].data_ptr(), la["ce"].data_ptr(),
                                                             la["cz"].data_ptr(), *ctx, *sizes))
    else:
        hip.check(lib.ditto_guided_update_packed_window(x.data_ptr(), e.data_ptr(), _ptr(la["z"]), _ptr(la["seeds"]), STEP, None,
                                                        la["a"].data_ptr(), la["ce"].data_ptr(), la["cz"].data_ptr(), *ctx, *sizes))


def _nan_guards(*pools):
    for pool in pools:
        assert torch.isnan(pool[:GUARD]).all() and torch.isnan(pool[-GUARD:]).all()


def _scratch_guards(dv):
    assert torch.all(dv["spool"][:GUARD_BYTES] == FILL) and torch.all(dv["spool"][-GUARD_BYTES:] == FILL)


@functools.lru_cache(maxsize=None)
def _launch1(name):
    """launch 1 on shape `name`, once: (batch, device buffers, pcoef) — shared and left unchanged by the tests that read it"""
    bt = Batch([(name, b) for b in range(4)])
    dv = bt.device()
    hip.check(project(bt, dv))
    return bt, dv, pcoef(bt, dv)


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_direction_and_coefficients(name):
    bt, dv, pc = _launch1(name)
    S = bt.S
    m_out = dv["m"].cpu()
    for k in range(bt.B):
        w, p_ = bt.window_np(k), bt.par[k]
        lo, hi = bt.win[k]
        m32, _ = R.direction32(*w, p_)
        assert np.array_equal(m_out[lo:hi].numpy().ravel().view(np.int32), m32.view(np.int32)), (name, k)
        bnd = R.bounds(*w, p_)
        for i, f in enumerate(("fx", "fc", "fd")):
            err = abs(float(pc[k, i]) - bnd["ref"][f])
            print(f"{name} utt {k} {f}: kernel {pc[k, i]!r} fp64 {bnd['ref'][f]!r} err {err:.3e} bound {bnd[f]:.3e}")
            assert err <= bnd[f], (name, k, f)
        assert pc[k, 3] == 0.0
    # the context rows of the direction, and everything that is only read, bit for bit; the guards; the scratch's unused slots
    ctx = ~bt.gen
    assert torch.equal(_bits(m_out[ctx]), _bits(bt.m_0[ctx]))
    assert torch.equal(_bits(dv["x2"].cpu()), _bits(bt.x2_0)) and torch.equal(_bits(dv["eps2"].cpu()), _bits(bt.eps2_0))
    _nan_guards(dv["x2_pool"], dv["eps2_pool"], dv["m_pool"])
    _scratch_guards(dv)
    part = dv["scratch"][hip.project_scratch_layout(bt.B):].cpu().view(torch.float64).view(bt.B, -1, 4)
    for k in range(bt.B):
        used = -(-((bt.win[k][1] - bt.win[k][0]) * bt.d // 4) // hip.RESCALE_CHUNK_QUADS)
        assert torch.all(part[k, :used, 3] == 0.0) and torch.isfinite(part[k, :used]).all()
        assert torch.all(part[k, used:].contiguous().view(torch.uint8) == FILL)


@pytest.mark.parametrize("line", LINES)
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_update_is_the_restated_chain_through_the_existing_entries(name, line):
    bt, dv, pc = _launch1(name)
    S, d = bt.S, bt.d
    la = line_args(bt, line)
    m_new = dv["m"].cpu()
    # e restated on the host from the kernel's own coefficients and direction
    e = torch.full((S, d), NAN)
    for k in range(bt.B):
        lo, hi = bt.win[k]
        x, c, u, m = bt.window_np(k)
        ek = R.e32(x, c, m_new[lo:hi].numpy(), pc[k])
        e[lo:hi] = torch.from_numpy(ek.reshape(hi - lo, d))
        bnd = R.bounds(x, c, u, m, bt.par[k])
        ratio = float(np.max(np.abs(ek.astype(np.float64) - bnd["ref"]["e"]) / bnd["e"]))
        print(f"{name} utt {k} e: largest error / bound {ratio:.3f}")
        assert ratio <= 1.0, (name, k)                          # (set 2: plain classifier-free guidance, u + w (c - u))
        if bt.par[k]["eta"] == 0.0 and bt.par[k]["beta"] == 0.0 and bt.par[k]["r"] == 0.0:
            Dc = bnd["ref"]["D"]
            Dh = bt.par[k]["kx"] * x.astype(np.float64).ravel() + bt.par[k]["ke"] * ek.astype(np.float64)
            dot, ob = abs(float((Dh - Dc) @ Dc)), R.ortho_bound(x, c, u, m, bt.par[k])
            print(f"{name} utt {k} orthogonality: |<D - D_c, D_c>| {dot:.3e} bound {ob:.3e} (|D - D_c| |D_c| = "
                  f"{float(np.linalg.norm(Dh - Dc) * np.linalg.norm(Dc)):.3e})")
            assert dot <= ob
    # the existing unguided entry on e
    x_ref, q_ref = bt.x2_0[:S].to(DEV), None if la["q"] is None else la["q"].clone()
    existing(bt, dv, la, x_ref, e.to(DEV), q_ref)
    # the project update: its eps2 holds c alone — the unconditional half is NaN in every row
    x2_pool, x2 = _guarded(bt.x2_0)
    eps_c = bt.eps2_0.clone()
    eps_c[S:] = NAN
    e_pool, eps2 = _guarded(eps_c)
    m_before = dv["m_pool"].clone()
    pcd = torch.from_numpy(pc).to(DEV)
    hip.check(update(bt, dv, la, x2, eps2, pcd))
    torch.cuda.synchronize()
    gen = bt.gen.to(DEV)
    for half in (x2[:S], x2[S:]):
        assert torch.equal(_bits(half[gen]), _bits(x_ref[gen])), (name, line)
        assert not torch.isnan(half[gen]).any()
    assert torch.equal(_bits(x2.cpu()[~bt.gen.repeat(2)]), _bits(bt.x2_0[~bt.gen.repeat(2)]))          # the context rows, both halves
    if q_ref is not None:
        assert torch.equal(_bits(la["q"]), _bits(q_ref))
        _nan_guards(la["q_pool"])
    if la["z"] is not None:
        _nan_guards(la["z_pool"])
    assert torch.equal(_bits(dv["m_pool"]), _bits(m_before)) and torch.equal(_bits(eps2.cpu()), _bits(eps_c))
    _nan_guards(x2_pool, e_pool)


def _run_all(bt, line, max_N=None, pl=None, ql=None):
    """launch 1 and the update of `line` on a fresh batch -> (pcoef, direction, x2, q) on the CPU"""
    dv = bt.device(max_N)
    hip.check(project(bt, dv, max_N=max_N, pl=pl, ql=ql))
    la = line_args(bt, line)
    hip.check(update(bt, dv, la, dv["x2"], dv["eps2"], dv["scratch"], max_N=max_N, pl=pl, ql=ql))
    pc = pcoef(bt, dv)
    _nan_guards(dv["x2_pool"], dv["eps2_pool"], dv["m_pool"])
    _scratch_guards(dv)
    return pc, dv["m"].cpu(), dv["x2"].cpu(), None if la["q"] is None else la["q"].cpu()


@pytest.mark.parametrize("line", ["philox", "ms_coefs"])
@pytest.mark.parametrize("name", ["d64", "d256"])
def test_an_utterance_depends_on_its_own_window_only(name, line):
    """an utterance's pcoef, direction, x' and q are the same bits at another position, in a batch of another B, and under any max_N
    the grid is sized by (Philox draws at the window-local index: the noise follows the utterance too)"""
    full = Batch([(name, b) for b in range(4)])
    base = _run_all(full, line)
    for order, max_N in (([3, 2, 1, 0], None), ([2, 0], None), ([1], None), ([0, 1, 2, 3], full.S), ([0, 1, 2, 3], 1)):
        bt = Batch([(name, b) for b in order])
        got = _run_all(bt, line, max_N=max_N)
        for k, b in enumerate(order):
            lo, hi = bt.win[k]
            blo, bhi = full.win[b]
            assert np.array_equal(got[0][k].view(np.int32), base[0][b].view(np.int32)), (order, max_N, b)
            assert torch.equal(_bits(got[1][lo:hi]), _bits(base[1][blo:bhi]))
            for off_g, off_b in ((0, 0), (bt.S, full.S)):
                assert torch.equal(_bits(got[2][off_g + lo:off_g + hi]), _bits(base[2][off_b + blo:off_b + bhi])), (order, max_N, b)
            if got[3] is not None:
                assert torch.equal(_bits(got[3][lo:hi]), _bits(base[3][blo:bhi]))


def test_bad_prompt_and_suffix_lengths_are_clamped():
    """P_b into [0, n_b - 1], then Q_b into [0, n_b - 1 - P_b]: wrong rows, never an access outside the utterance's own"""
    name, order = "d256", [0, 1, 2, 3]
    n = [sum(R.SHAPES[name][1][b]) for b in order]              # 10, 68, 72, 28 rows
    bad_p, bad_q = [-3, n[1] + 5, 2, 0x7fffffff], [100, 7, -9, -0x80000000]
    want = [(0, n[0] - 1), (n[1] - 1, 0), (2, 0), (n[3] - 1, 0)]                                        # (P, Q) after the clamps
    outs = []
    for lens, pl, ql in ((want, None, None), (want, _i32(bad_p), _i32(bad_q))):
        bt = Batch([(name, b) for b in order], clean=True, lens=[(n[k] - p - q, p, q) for k, (p, q) in enumerate(lens)])
        outs.append(_run_all(bt, "ms1", pl=pl, ql=ql))
    for a, b in zip(*outs):
        assert torch.equal(_bits(torch.as_tensor(a)), _bits(torch.as_tensor(b)))


def test_refused_calls_touch_nothing():
    bt = Batch([("d256", b) for b in range(4)])
    dv = bt.device()
    lib = hip.lib()
    la = line_args(bt, "none")
    lm = line_args(bt, "ms1")
    pcd = torch.zeros(bt.B, 4, device=DEV)
    for rc, code in ((project(bt, dv, d=bt.d + 32), hip.ERR_SHAPE), (project(bt, dv, max_N=bt.S + 1), hip.ERR_SHAPE),
                     (project(bt, dv, B=0), hip.ERR_SHAPE), (project(bt, dv, proj=None), hip.ERR_ARG),
                     (project(bt, dv, dir=None), hip.ERR_ARG), (project(bt, dv, cu=None), hip.ERR_ARG),
                     (project(bt, dv, scratch=dv["scratch"].data_ptr() + 16), hip.ERR_ARG),
                     (project(bt, dv, scratch_bytes=dv["need"] - 1), hip.ERR_SIZE),
                     (project(bt, dv, proj=dv["proj"].data_ptr() + 8), hip.ERR_ARG),
                     (update(bt, dv, la, dv["x2"], dv["eps2"], pcd, pcoef=None), hip.ERR_ARG),
                     (update(bt, dv, la, dv["x2"], dv["eps2"], pcd, a=None), hip.ERR_ARG),
                     (update(bt, dv, la, dv["x2"], dv["eps2"], pcd, noise=dv["m"].data_ptr(), seeds=dv["cu"].data_ptr()), hip.ERR_ARG),
                     (update(bt, dv, la, dv["x2"], dv["eps2"], pcd, d=96), hip.ERR_SHAPE),
                     (update(bt, dv, lm, dv["x2"], dv["eps2"], pcd, q=None), hip.ERR_ARG),
                     (update(bt, dv, lm, dv["x2"], dv["eps2"], pcd, step=None), hip.ERR_ARG),
                     (update(bt, dv, lm, dv["x2"], dv["eps2"], pcd, coefs=dv["proj"].data_ptr()), hip.ERR_ARG),
                     (update(bt, dv, lm, dv["x2"], dv["eps2"], pcd, B=70000), hip.ERR_SHAPE)):
        assert rc == code, lib.ditto_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(dv["x2"].cpu()), _bits(bt.x2_0)) and torch.equal(_bits(dv["m"].cpu()), _bits(bt.m_0))
    assert torch.all(dv["spool"] == FILL) and torch.all(pcd == 0)
