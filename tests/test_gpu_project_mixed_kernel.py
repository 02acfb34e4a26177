"""-m gpu: projected guidance over a request stream's mixed layout (csrc/guided_project_mixed.hip) through the C entries of
include/ditto_project_stream.h, on tests/project_ref.py's inputs.

Batch "d64": B = 5 at d = 64 with kinds [3, 0, 1, 3, 3]; the projected utterances take project_ref.SHAPES["d64"]'s windows of 1 row, 256
rows (exactly one chunk of 4096 quads) and 257 rows, the last behind a prompt; one runs use_prev = 0 over a NaN-filled direction, one
beta = -0.5 with use_prev = 1 and the threshold ACTIVE (r = 0.5 against an RMS of about 1.1: the reference's rho < 1 is asserted), one
eta = 1 with r off and beta = 0.  Batch "d768": B = 3 at d = 768 with kinds [1, 3, 0] and the 22-row window, where a chunk boundary falls
inside a row.  NaN guard rows stand around every buffer, the scratch stands between filled bands, and NaN stands in every row the
contract says is not read: prompt rows, the direction's rows of kinds 0 and 1, and the copy region's rows that belong to nobody (a gap
between two copies and spare rows behind the last).

Held, in the three noise modes: a projected utterance's pcoef, m' and x' — in its own rows and its copy's — bit-equal to
ditto_guidance_project_packed + ditto_guided_update_packed_project (tags form) run on that utterance alone in a [2n, d] batch, and its
pcoef inside project_ref.bounds; the rows of kinds 1 and 0 bit-equal to ditto_guided_update_packed_mixed on the same buffers, their
pcoef (0, 1, 0, 0); everything else untouched, compared as int32; the same bits with the utterances permuted, in another B, and with
max_N exact, over- and under-reported; kind 7, and kind 3 without a partner, behave as kind 0; refused calls change no byte."""
import functools

import numpy as np
import pytest
import torch

import project_ref as R
from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, GUARD_BYTES, FILL = 4, 512, 0xA5
NAN = float("nan")
MODES = ["philox", "buffer", "none"]
PROJECT, CFG, PLAIN = hip.KIND_PROJECT, hip.KIND_CFG, hip.KIND_PLAIN

# uid -> (d, kind, project_ref shape and utterance or None for hashed rows, generated rows, prompt rows, parameters or None)
UTTS = {
    0: (64, PROJECT, ("d64", 0), 1, 0, R.par(R.KX_V, R.KE_V, 4.0, 0.0, r=0.25, beta=0.0, use_prev=0)),       # NaN direction, never read
    1: (64, PLAIN, None, 5, 2, None),
    2: (64, CFG, None, 7, 0, None),
    3: (64, PROJECT, ("d64", 1), 256, 0, R.par(R.KX_EPS, R.KE_EPS, 5.0, 0.3, r=0.5, beta=-0.5, use_prev=1)),
    4: (64, PROJECT, ("d64", 2), 257, 3, R.par(R.KX_EPS, R.KE_EPS, 5.0, 1.0, r=0.0, beta=0.0, use_prev=1)),
    5: (768, CFG, None, 4, 0, None),
    6: (768, PROJECT, ("d768", 0), 22, 0, R.par(R.KX_V, R.KE_V, 4.0, 0.0, r=0.25, beta=0.0, use_prev=0)),
    7: (768, PLAIN, None, 3, 1, None),
}
BATCHES = {"d64": [0, 1, 2, 3, 4], "d768": [5, 6, 7]}
# the solver's per-utterance arguments follow the utterance: a, ce, cz (one of them 0: no draw), w, seed, tag
LINE = {u: (0.9 - 0.02 * u, -0.3 + 0.07 * u, 0.0 if u in (2, 4) else 0.2 + 0.05 * u, 2.0 + 0.5 * u, 11 + u, 900 + u) for u in UTTS}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(t):
    g = torch.full((GUARD, t.shape[1]), NAN)
    pool = torch.cat([g, t, g]).to(DEV).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


@functools.lru_cache(maxsize=None)
def data(uid):
    """(x, c, u, m, z) fp32 torch [g, d] over the utterance's generated window; m is NaN unless it is projected with use_prev"""
    d, kind, ref, g, _, par = UTTS[uid]
    if ref is not None:
        assert R.SHAPES[ref[0]][0] == d and R.SHAPES[ref[0]][1][ref[1]] == (g, 0, 0)
        x, c, u, m = (torch.from_numpy(v.copy()) for v in R.rows(*ref))
    else:
        x, c, nz = (hash_normal((g, d), tag, 7000 + uid) for tag in ("pm_x", "pm_c", "pm_u"))
        u, m = 0.8 * c + 0.6 * nz, torch.full((g, d), NAN)
    if par is None or not par["use_prev"]:
        m = torch.full((g, d), NAN)
    assert par is None or not par["use_prev"] or torch.isfinite(m).all()
    return x, c, u, m, hash_normal((g, d), "pm_z", 7000 + uid)


class Mixed:
    """the utterances `uids` packed in that order in the mixed layout.  `kinds`: what the kernels are told (default: the utterances'
    own); `partnered`: which utterances get a copy (default: kind 1 or 3).  The copies stand in batch order behind row S with a gap of
    2 rows behind the first and 3 spare rows behind the last, all NaN (fewer where S_G <= S leaves no room for them)"""

    def __init__(self, uids, kinds=None, partnered=None):
        self.uids, self.B = list(uids), len(uids)
        self.d = UTTS[uids[0]][0]
        self.kinds = [UTTS[u][1] for u in uids] if kinds is None else list(kinds)
        own = [UTTS[u][1] != PLAIN for u in uids] if partnered is None else list(partnered)
        self.g, self.P = [UTTS[u][3] for u in uids], [UTTS[u][4] for u in uids]
        self.n = [g + p for g, p in zip(self.g, self.P)]
        self.cu = [0]
        for n in self.n:
            self.cu.append(self.cu[-1] + n)
        S = self.S = self.cu[-1]
        self.max_N = max(self.n)
        room = S - sum(n for n, f in zip(self.n, own) if f)      # S_G <= S: the gap and the spare rows take what is left, at most 2 + 3
        gap = min(2, room) if sum(own) > 1 else 0
        self.partner, starts, at = [], [], S
        for k in range(self.B):
            self.partner.append(len(starts) if own[k] else -1)
            if own[k]:
                starts.append(at)
                at += self.n[k] + (gap if len(starts) == 1 else 0)
        self.G = len(starts)
        self.S_G = (at + min(3, room - gap) - S) if self.G else 0
        self.offsets = self.cu + (starts[1:] + [S + self.S_G] if self.G else [])
        assert len(self.offsets) == self.B + self.G + 1 and self.S_G <= S
        d = self.d
        rows = S + self.S_G
        x2, eps2, m, z = (torch.full((r, d), NAN) for r in (rows, rows, S, S))
        self.win, self.cwin = [], []
        for k, u in enumerate(self.uids):
            x, c, uu, mm, zz = data(u)
            lo, hi = self.cu[k] + self.P[k], self.cu[k + 1]
            x2[lo:hi], eps2[lo:hi], z[lo:hi] = x, c, zz
            if UTTS[u][1] == PROJECT:
                m[lo:hi] = mm
            self.win.append((lo, hi))
            if own[k]:
                clo = starts[self.partner[k]] + self.P[k]
                x2[clo:clo + self.g[k]], eps2[clo:clo + self.g[k]] = x, uu
                self.cwin.append((clo, clo + self.g[k]))
            else:
                self.cwin.append(None)
        self.x2_0, self.eps2_0, self.m_0, self.z_0 = x2, eps2, m, z
        self.proj = torch.zeros(self.B, 8)
        for k, u in enumerate(self.uids):
            p_ = UTTS[u][5]
            if p_ is None:
                self.proj[k] = NAN                               # read for kind 3 only
                continue
            self.proj[k, :6] = torch.tensor([p_[f] for f in R.PAR_FIELDS[:6]])
            self.proj.view(torch.int32)[k, 6] = p_["use_prev"]
            self.proj[k, 7] = 0.0

    def device(self, mode, max_N=None):
        dv = dict(proj=self.proj.to(DEV), cu=_i32(self.offsets), partner=_i32(self.partner), kind=_i32(self.kinds), pl=_i32(self.P))
        for name, t in (("x2", self.x2_0), ("eps2", self.eps2_0), ("m", self.m_0), ("z", self.z_0)):
            dv[name + "_pool"], dv[name] = _guarded(t)
        per = lambda i, dtype=torch.float32: torch.tensor([LINE[u][i] for u in self.uids], dtype=dtype, device=DEV)
        dv.update(a=per(0), ce=per(1), cz=per(2), w=per(3), seeds=per(4, torch.int64), tags=per(5, torch.int32))
        dv["noise"] = dict(noise=dv["z"].data_ptr() if mode == "buffer" else None, seeds=dv["seeds"].data_ptr() if mode == "philox" else None,
                           tags=dv["tags"].data_ptr() if mode == "philox" else None)
        need = hip.lib().ditto_guidance_project_bytes(self.B, max(self.max_N, max_N or 0), self.d)
        assert need > 0
        dv["need"] = need
        dv["spool"] = torch.full((need + 2 * GUARD_BYTES,), FILL, dtype=torch.uint8, device=DEV)
        dv["scratch"] = dv["spool"][GUARD_BYTES:GUARD_BYTES + need]
        assert dv["scratch"].data_ptr() % 256 == 0
        return dv

    def layout(self, dv, max_N=None):
        return dict(cu=dv["cu"].data_ptr(), partner=dv["partner"].data_ptr(), prompt_len=dv["pl"].data_ptr(), B=self.B, G=self.G, S=self.S,
                    S_G=self.S_G, max_N=self.max_N if max_N is None else max_N, d=self.d, stream=_s())


def launch1(bt, dv, max_N=None, **over):
    a = dict(x2=dv["x2"].data_ptr(), eps2=dv["eps2"].data_ptr(), dir=dv["m"].data_ptr(), proj=dv["proj"].data_ptr(),
             kind=dv["kind"].data_ptr(), scratch=dv["scratch"].data_ptr(), scratch_bytes=dv["need"], **bt.layout(dv, max_N))
    a.update(over)
    return hip.call("ditto_guidance_project_packed_mixed", **a)


def launch2(bt, dv, max_N=None, **over):
    a = dict(x2=dv["x2"].data_ptr(), eps2=dv["eps2"].data_ptr(), dir=dv["m"].data_ptr(), pcoef=dv["scratch"].data_ptr(),
             kind=dv["kind"].data_ptr(), w=dv["w"].data_ptr(), a=dv["a"].data_ptr(), ce=dv["ce"].data_ptr(), cz=dv["cz"].data_ptr(),
             **dv["noise"], **bt.layout(dv, max_N))
    a.update(over)
    return hip.call("ditto_guided_update_packed_project_mixed", **a)


def run(bt, mode, max_N=None):
    """both launches on fresh buffers -> (pcoef numpy [B, 4], dir, x2 on the CPU, the device buffers)"""
    dv = bt.device(mode, max_N)
    hip.check(launch1(bt, dv, max_N))
    hip.check(launch2(bt, dv, max_N))
    torch.cuda.synchronize()
    pc = dv["scratch"][:16 * bt.B].view(torch.float32).view(bt.B, 4).cpu().numpy()
    return pc, dv["m"].cpu(), dv["x2"].cpu(), dv


@functools.lru_cache(maxsize=None)
def solo(uid, mode):
    """the closed entries on utterance `uid` alone in a [2n, d] batch: ditto_guidance_project_packed, then
    ditto_guided_update_packed_project in its tags form -> (pcoef numpy [4], m' [g, d], x' of the conditional half [g, d], of the
    unconditional half [g, d]).  Computed once per utterance and noise mode and left unchanged"""
    d, _, _, g, P, p_ = UTTS[uid]
    n = g + P
    x, c, u, m, z = data(uid)
    pad = lambda t: torch.cat([torch.full((P, d), NAN), t])
    x2 = torch.cat([pad(x), pad(x)]).to(DEV)
    eps2 = torch.cat([pad(c), pad(u)]).to(DEV)
    mm, zz = pad(m).to(DEV), pad(z).to(DEV)
    proj = torch.zeros(1, 8)
    proj[0, :6] = torch.tensor([p_[f] for f in R.PAR_FIELDS[:6]])
    proj.view(torch.int32)[0, 6] = p_["use_prev"]
    proj = proj.to(DEV)
    need = hip.lib().ditto_guidance_project_bytes(1, n, d)
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    scratch = scratch[(-scratch.data_ptr()) % 256:][:need]
    cu, pl = _i32([0, n]), _i32([P])
    rows = dict(cu=cu.data_ptr(), prompt_len=pl.data_ptr(), suffix_len=None, B=1, S=n, max_N=n, d=d, stream=_s())
    hip.check(hip.call("ditto_guidance_project_packed", x2=x2.data_ptr(), eps2=eps2.data_ptr(), dir=mm.data_ptr(), proj=proj.data_ptr(),
                       scratch=scratch.data_ptr(), scratch_bytes=need, **rows))
    a_, ce, cz, _, seed, tag = LINE[uid]
    a_, ce, cz = _f32([a_]), _f32([ce]), _f32([cz])
    seeds, tags = torch.tensor([seed], dtype=torch.int64, device=DEV), _i32([tag])
    hip.check(hip.call("ditto_guided_update_packed_project", x2=x2.data_ptr(), eps2=eps2.data_ptr(), dir=mm.data_ptr(),
                       pcoef=scratch.data_ptr(), noise=zz.data_ptr() if mode == "buffer" else None,
                       seeds=seeds.data_ptr() if mode == "philox" else None, step=0, tags=tags.data_ptr(), a=a_.data_ptr(),
                       ce=ce.data_ptr(), cz=cz.data_ptr(), **rows))
    torch.cuda.synchronize()
    return (scratch[:16].view(torch.float32).cpu().numpy().copy(), mm[P:].cpu(), x2[P:n].cpu(), x2[n + P:].cpu())


def mixed_reference(bt, mode, partner):
    """ditto_guided_update_packed_mixed on the same buffers with the partner table `partner` -> x2 on the CPU"""
    dv = bt.device(mode)
    pt = _i32(partner)
    lay = bt.layout(dv)
    lay["partner"] = pt.data_ptr()
    nz = dict(dv["noise"])
    if mode != "philox":
        nz["tags"] = dv["tags"].data_ptr()
    hip.check(hip.call("ditto_guided_update_packed_mixed", x2=dv["x2"].data_ptr(), eps2=dv["eps2"].data_ptr(), **nz, w=dv["w"].data_ptr(),
                       a=dv["a"].data_ptr(), ce=dv["ce"].data_ptr(), cz=dv["cz"].data_ptr(), **lay))
    torch.cuda.synchronize()
    return dv["x2"].cpu()


def _untouched(bt, dv, x2, m, written_x, written_m):
    """every row outside `written_x` / `written_m` holds its first bits; eps2, the noise buffer, the guards and the scratch's bands too"""
    keep = torch.ones(bt.S + bt.S_G, dtype=torch.bool)
    for lo, hi in written_x:
        keep[lo:hi] = False
    assert torch.equal(_bits(x2[keep]), _bits(bt.x2_0[keep]))
    keep = torch.ones(bt.S, dtype=torch.bool)
    for lo, hi in written_m:
        keep[lo:hi] = False
    assert torch.equal(_bits(m[keep]), _bits(bt.m_0[keep]))
    assert torch.equal(_bits(dv["eps2"].cpu()), _bits(bt.eps2_0)) and torch.equal(_bits(dv["z"].cpu()), _bits(bt.z_0))
    for name in ("x2", "eps2", "m", "z"):
        pool = dv[name + "_pool"]
        assert torch.isnan(pool[:GUARD]).all() and torch.isnan(pool[-GUARD:]).all(), name
    assert torch.all(dv["spool"][:GUARD_BYTES] == FILL) and torch.all(dv["spool"][-GUARD_BYTES:] == FILL)


def _check(bt, mode, got, eff=None):
    """`got` = run()'s result against the solo runs (effective kind 3), the mixed entry (1 and 0) and the untouched rows; `eff`: the
    kinds the kernels are expected to act on (default: the ones they were told)"""
    pc, m, x2, dv = got
    eff = bt.kinds if eff is None else eff
    ref = mixed_reference(bt, mode, [p if k in (CFG, PROJECT) else -1 for p, k in zip(bt.partner, eff)])
    written_x, written_m = [], []
    for k, u in enumerate(bt.uids):
        lo, hi = bt.win[k]
        written_x.append((lo, hi))
        if eff[k] == PROJECT:
            spc, sm, sxc, sxu = solo(u, mode)
            clo, chi = bt.cwin[k]
            assert np.array_equal(pc[k].view(np.int32), spc.view(np.int32)), (u, pc[k], spc)
            assert torch.equal(_bits(m[lo:hi]), _bits(sm)), u
            assert torch.equal(_bits(x2[lo:hi]), _bits(sxc)) and torch.equal(_bits(x2[clo:chi]), _bits(sxu)), u
            assert torch.isfinite(x2[lo:hi]).all() and torch.isfinite(m[lo:hi]).all()
            written_x.append((clo, chi))
            written_m.append((lo, hi))
        else:
            assert np.array_equal(pc[k], np.array([0.0, 1.0, 0.0, 0.0], np.float32)), (u, pc[k])
            assert torch.equal(_bits(x2[lo:hi]), _bits(ref[lo:hi])), u
            assert torch.isfinite(x2[lo:hi]).all()
            if eff[k] == CFG:
                clo, chi = bt.cwin[k]
                assert torch.equal(_bits(x2[clo:chi]), _bits(ref[clo:chi])) and torch.equal(_bits(x2[clo:chi]), _bits(x2[lo:hi])), u
                written_x.append((clo, chi))
    _untouched(bt, dv, x2, m, written_x, written_m)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_three_kinds_in_one_step(name, mode):
    bt = Mixed(BATCHES[name])
    got = run(bt, mode)
    _check(bt, mode, got)
    for k, u in enumerate(bt.uids):                              # the coefficients inside the derived bounds against fp64
        p_ = UTTS[u][5]
        if p_ is None:
            continue
        x, c, uu, m, _ = (t.numpy() for t in data(u))
        bnd = R.bounds(x, c, uu, m, p_)
        for i, f in enumerate(("fx", "fc", "fd")):
            err = abs(float(got[0][k, i]) - bnd["ref"][f])
            print(f"{name} utt {u} {f}: kernel {got[0][k, i]!r} fp64 {bnd['ref'][f]!r} err {err:.3e} bound {bnd[f]:.3e}")
            assert err <= bnd[f], (name, u, f)
        if u == 3:
            assert bnd["ref"]["rho"] < 0.75                      # the threshold is active, well away from its edge


@pytest.mark.parametrize("mode", MODES)
def test_an_utterance_depends_on_its_own_window_only(mode):
    """permuted, in another B, and under max_N exact, over-reported (S) and under-reported (1: one grid column strides over all of an
    utterance's chunks): the solo runs and the mixed entry are the reference every time"""
    full = BATCHES["d64"]
    for order, max_N in (([4, 3, 2, 1, 0], None), ([3, 1], None), ([4], None), (full, "S"), (full, 1), ([2, 4, 0], 1)):
        bt = Mixed(order)
        _check(bt, mode, run(bt, mode, bt.S if max_N == "S" else max_N))


@pytest.mark.parametrize("mode", MODES)
def test_kind_clamps(mode):
    """a value outside {1, 3} counts as 0 even with a partner; a 3 (or a 1) without a usable partner counts as 0"""
    uids = BATCHES["d64"]
    own = [UTTS[u][1] != PLAIN for u in uids]
    bt = Mixed(uids, kinds=[7, 2, -1, PROJECT, PROJECT], partnered=own)
    _check(bt, mode, run(bt, mode), eff=[PLAIN, PLAIN, PLAIN, PROJECT, PROJECT])
    bt = Mixed(uids, kinds=[PROJECT, PLAIN, CFG, PROJECT, PROJECT], partnered=[False, False, False, True, False])
    _check(bt, mode, run(bt, mode), eff=[PLAIN, PLAIN, PLAIN, PROJECT, PLAIN])


def test_refused_calls_change_no_byte():
    bt = Mixed(BATCHES["d64"])
    dv = bt.device("none")
    before = {k: dv[k].clone() for k in ("x2_pool", "eps2_pool", "m_pool", "z_pool", "spool")}
    lib = hip.lib()
    cases = [(launch1(bt, dv, d=96), hip.ERR_SHAPE), (launch1(bt, dv, max_N=bt.S + 1), hip.ERR_SHAPE), (launch1(bt, dv, B=0), hip.ERR_SHAPE),
             (launch1(bt, dv, G=bt.B + 1), hip.ERR_SHAPE), (launch1(bt, dv, S_G=0), hip.ERR_SHAPE), (launch1(bt, dv, S_G=bt.S + 1), hip.ERR_SHAPE),
             (launch1(bt, dv, proj=None), hip.ERR_ARG), (launch1(bt, dv, dir=None), hip.ERR_ARG), (launch1(bt, dv, kind=None), hip.ERR_ARG),
             (launch1(bt, dv, partner=None), hip.ERR_ARG), (launch1(bt, dv, cu=None), hip.ERR_ARG),
             (launch1(bt, dv, proj=dv["proj"].data_ptr() + 8), hip.ERR_ARG), (launch1(bt, dv, dir=dv["m"].data_ptr() + 4), hip.ERR_ARG),
             (launch1(bt, dv, scratch=dv["scratch"].data_ptr() + 16), hip.ERR_ARG),
             (launch1(bt, dv, scratch_bytes=dv["need"] - 1), hip.ERR_SIZE),
             (launch2(bt, dv, pcoef=None), hip.ERR_ARG), (launch2(bt, dv, pcoef=dv["scratch"].data_ptr() + 4), hip.ERR_ARG),
             (launch2(bt, dv, w=None), hip.ERR_ARG), (launch2(bt, dv, a=None), hip.ERR_ARG), (launch2(bt, dv, kind=None), hip.ERR_ARG),
             (launch2(bt, dv, noise=dv["z"].data_ptr(), seeds=dv["seeds"].data_ptr(), tags=dv["tags"].data_ptr()), hip.ERR_ARG),
             (launch2(bt, dv, seeds=dv["seeds"].data_ptr()), hip.ERR_ARG), (launch2(bt, dv, noise=dv["z"].data_ptr() + 4), hip.ERR_ARG),
             (launch2(bt, dv, d=96), hip.ERR_SHAPE), (launch2(bt, dv, G=0), hip.ERR_SHAPE), (launch2(bt, dv, B=70000), hip.ERR_SHAPE)]
    for i, (rc, code) in enumerate(cases):
        assert rc == code, (i, rc, lib.ditto_last_error())
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(dv[k].view(torch.uint8), t.view(torch.uint8)), k
