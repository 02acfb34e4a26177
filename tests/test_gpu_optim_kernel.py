"""The fused optimizer's C entries (include/ditto_optim.h, csrc/optim.hip) on guarded buffers: every tensor of the case of
tests/optim_ref.py (sizes 1, 3, 4, 5, 1023, one chunk, one chunk + 1, three chunks + 5; two lr / weight-decay groups; one segment
without an average) stands between guard bands of NaNs — directly behind its last element, so the whole-quad read of a tail sees them.
The norm against the float64 sum, its bits under smaller grids; p', m', v', ema' inside the bounds optim_ref derives at steps 1 - 3;
clip exactly 1 and the one-launch step bit-equal to the three-launch one when nothing is clipped; a step with a NaN / an inf in one
gradient element skipped without a trace; the swap; the refusals.  Guard bands intact throughout."""
import struct

import numpy as np
import pytest
import torch

import optim_ref as R
from ditto_tts_amd import hip, optim
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                       # fp32 words in front of and behind every tensor
SENT = 0x7FC00BAD                # a quiet NaN: arithmetic on a guard word poisons whatever it reaches
KINDS = ("p", "g", "m", "v", "ema")
N = len(R.CASE_SIZES)


class Bank:
    """one buffer per kind; tensor i of every kind at offs[i] (16-byte aligned), GUARD sentinel words around it"""

    def __init__(self):
        self.offs, end = [], 0
        for n in R.CASE_SIZES:
            o = (end + GUARD + 3) // 4 * 4
            self.offs.append(o)
            end = o + n
        self.total = end + GUARD
        self.buf = {k: torch.full((self.total,), SENT, dtype=torch.int32, device=DEV).view(torch.float32) for k in KINDS}
        guard = torch.ones(self.total, dtype=torch.bool)
        for o, n in zip(self.offs, R.CASE_SIZES):
            guard[o:o + n] = False
        self.guard = guard.to(DEV)
        p, ema = R.case_params()
        self.put("p", p), self.put("ema", ema)
        self.put("m", [torch.zeros(n) for n in R.CASE_SIZES]), self.put("v", [torch.zeros(n) for n in R.CASE_SIZES])
        self.state = torch.frombuffer(bytearray(optim.state_block(*R.CASE_BETAS, 0)), dtype=torch.uint8).to(DEV)
        self.scratch = torch.full((64,), float("nan"), dtype=torch.float64, device=DEV)
        self.table = torch.empty(N * 72, dtype=torch.uint8, device=DEV)
        self.phase = 0

    def put(self, kind, tensors):
        for o, t in zip(self.offs, tensors):
            self.buf[kind][o:o + t.numel()] = t.to(DEV)

    def get(self, kind):
        return [self.buf[kind][o:o + n].cpu() for o, n in zip(self.offs, R.CASE_SIZES)]

    def bits(self):
        return {k: self.buf[k].view(torch.int32).clone() for k in KINDS}

    def guards_intact(self):
        return all(bool(torch.all(self.buf[k].view(torch.int32)[self.guard] == SENT)) for k in KINDS)

    def upload_table(self, ema=True):
        rows = np.zeros(N, dtype=optim.SEG_DTYPE)
        addr = {k: [self.buf[k].data_ptr() + 4 * o for o in self.offs] for k in KINDS}
        e = [a if ema and i != R.CASE_NO_EMA else 0 for i, a in enumerate(addr["ema"])]
        lrwd = [R.case_lr_wd(i) for i in range(N)]
        self.n_chunks = optim.fill_table(rows, (addr["p"], addr["g"], addr["m"], addr["v"], e), list(R.CASE_SIZES),
                                         [a for a, _ in lrwd], [b for _, b in lrwd])
        self.table.copy_(torch.from_numpy(rows.view(np.uint8).copy()))

    def state_host(self):
        raw = bytes(self.state.cpu().numpy())
        slots = [struct.unpack_from("<ddqq", raw, 32 * k) for k in range(2)]
        norm, norm32, clip, skip = struct.unpack_from("<dffi", raw, 64)
        return slots, norm, norm32, clip, skip

    def step(self, hyper, grid_limit=0):
        normed = hyper.max_norm > 0 or hyper.skip_nonfinite
        rc = hip.call("ditto_optim_adamw_step", table=self.table.data_ptr(), n_seg=N, n_chunks=self.n_chunks, hyper=hyper,
                      state=self.state.data_ptr(), phase=self.phase, scratch=self.scratch.data_ptr() if normed else None,
                      scratch_bytes=self.scratch.numel() * 8 if normed else 0, grid_limit=grid_limit, stream=stream())
        hip.check(rc)
        self.phase += 1
        torch.cuda.synchronize()

    def slot(self):
        """the slot the last step wrote"""
        return self.state_host()[0][self.phase & 1]


def _hyper(max_norm=0.0, skip=0):
    return hip.OptimHyper(*R.CASE_BETAS, R.CASE_EPS, max_norm, R.CASE_DECAY, skip, 0)


def _check_step(bank, before, grads, step, clip_ref, tag):
    worst = {}
    for kind in ("p", "m", "v", "ema"):
        got = bank.get(kind)
        for i in range(N):
            lr, wd = R.case_lr_wd(i)
            ema_b = None if i == R.CASE_NO_EMA else before["ema"][i]
            want, bound = R.chain_fp64(before["p"][i], grads[i], before["m"][i], before["v"][i], ema_b, step, lr, wd, clip=clip_ref)
            if kind == "ema" and ema_b is None:
                assert torch.equal(got[i], before["ema"][i]), f"{tag}: the segment without an average had its buffer written"
                continue
            r = R.worst_ratio(got[i], want[kind], bound[kind])
            worst[kind] = max(worst.get(kind, 0.0), r)
            assert r <= 1.0, f"{tag} step {step}: {kind} of segment {i} (n = {R.CASE_SIZES[i]}) at {r:.3f} of its bound"
    print(f"{tag} step {step}: worst ratio to the bound {worst}")


def _three_steps(bank, hyper, max_norm, tag, grid_limit=0):
    bank.upload_table()
    for step in range(1, R.CASE_STEPS + 1):
        grads = R.case_grads(step)
        bank.put("g", grads)
        before = {k: bank.get(k) for k in ("p", "m", "v", "ema")}
        bank.step(hyper, grid_limit)
        clip_ref = R.clip_factor(R.global_norm(grads), max_norm)
        _check_step(bank, before, grads, step, clip_ref, tag)
        _, _, _, clip, skip = bank.state_host()
        assert skip == 0 and abs(clip - clip_ref) <= 2 * R.U32 * clip_ref, (clip, clip_ref)
        if step == 1 and clip_ref == 1.0:          # gs = g bit for bit: with m = 0, m' is the one product fl(1 - b1) g
            for g, m in zip(grads, bank.get("m")):
                assert np.array_equal(m.numpy(), (np.float32(1.0 - R.CASE_BETAS[0]) * g.numpy()).astype(np.float32))
        assert bank.guards_intact(), f"{tag} step {step}: a guard band was written"
    b1p = b2p = 1.0
    for _ in range(R.CASE_STEPS):
        b1p, b2p = b1p * R.CASE_BETAS[0], b2p * R.CASE_BETAS[1]
    assert bank.slot() == (b1p, b2p, R.CASE_STEPS, 0), bank.state_host()


def test_norm_within_its_bound_and_the_same_bits_under_smaller_grids():
    bank = Bank()
    bank.upload_table()
    grads = R.case_grads(1)
    bank.put("g", grads)
    want = R.global_norm(grads)
    n = sum(R.CASE_SIZES)
    seen = []
    for grid_limit in (0, 1, 3, 5):
        bank.scratch.fill_(float("nan"))
        hip.check(hip.call("ditto_optim_grad_norm", table=bank.table.data_ptr(), n_seg=N, n_chunks=bank.n_chunks,
                           hyper=_hyper(R.CASE_MAX_NORM, 1), state=bank.state.data_ptr(), scratch=bank.scratch.data_ptr(),
                           scratch_bytes=bank.scratch.numel() * 8, grid_limit=grid_limit, stream=stream()))
        torch.cuda.synchronize()
        slots, norm, norm32, clip, skip = bank.state_host()
        seen.append(struct.pack("<d", norm))
        assert abs(norm - want) <= R.norm_rtol(n) * want, (norm, want)
        assert norm32 == float(np.float32(norm)) and skip == 0
        assert clip == float(np.float32(min(1.0, R.CASE_MAX_NORM / (norm + 1e-6))))      # the formula, in fp64, rounded once
        assert slots[0] == slots[1] == (1.0, 1.0, 0, 0)                                   # the norm alone advances nothing
    assert len(set(seen)) == 1, seen
    assert bank.n_chunks == 12 and bool(torch.isnan(bank.scratch[bank.n_chunks:]).all())  # one partial per chunk, none behind them
    assert bank.guards_intact()


def test_three_steps_inside_the_bounds_with_clipping_active():
    a, b = Bank(), Bank()
    _three_steps(a, _hyper(R.CASE_MAX_NORM, 0), R.CASE_MAX_NORM, "clip 10")
    _three_steps(b, _hyper(R.CASE_MAX_NORM, 1), R.CASE_MAX_NORM, "clip 10, 2 workgroups", grid_limit=2)
    for k in KINDS:
        assert torch.equal(a.buf[k].view(torch.int32), b.buf[k].view(torch.int32)), f"{k}: the bits depend on the grid"


def test_clip_is_exactly_one_and_one_launch_equals_three_when_nothing_is_clipped():
    off, large = Bank(), Bank()
    _three_steps(off, _hyper(0.0, 0), None, "clip off")                   # one launch a step
    _three_steps(large, _hyper(1e3, 0), 1e3, "max_norm 1e3")              # norm ~36: three launches, clip = 1
    assert large.state_host()[3] == 1.0 and off.state_host()[3] == 1.0
    for k in KINDS:
        assert torch.equal(off.buf[k].view(torch.int32), large.buf[k].view(torch.int32)), k
    assert off.slot() == large.slot()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_step_is_skipped_without_a_trace(bad):
    hyper = _hyper(R.CASE_MAX_NORM, 1)
    a, b = Bank(), Bank()
    for bank in (a, b):
        bank.upload_table()
        bank.put("g", R.case_grads(1))
        bank.step(hyper)
    g = R.case_grads(2)
    g[6][R.CHUNK] = bad                                     # the one-element tail chunk of the one-chunk + 1 segment
    b.put("g", g)
    before, slot = b.bits(), b.slot()
    b.step(hyper)
    after = b.bits()
    for k in KINDS:
        assert torch.equal(before[k], after[k]), f"{k} changed in a skipped step"
    slots, norm, _, _, skip = b.state_host()
    assert skip == 1 and not np.isfinite(norm)
    assert b.slot() == slot[:3] + (slot[3] + 1,) == (R.CASE_BETAS[0], R.CASE_BETAS[1], 1, 1)
    for bank in (a, b):                                     # the following clean step: as if nothing had happened
        bank.put("g", R.case_grads(2))
        bank.step(hyper)
    for k in KINDS:
        assert torch.equal(a.buf[k].view(torch.int32), b.buf[k].view(torch.int32)), k
    assert a.slot()[:3] == b.slot()[:3] and a.slot()[2] == 2 and (a.slot()[3], b.slot()[3]) == (0, 1)
    assert a.state_host()[1:] == b.state_host()[1:]
    assert a.guards_intact() and b.guards_intact()


@pytest.mark.parametrize("grid_limit", [0, 1])
def test_swap_exchanges_bits_and_twice_is_the_identity(grid_limit):
    bank = Bank()
    bank.upload_table()
    before = bank.bits()
    swap = lambda: hip.check(hip.call("ditto_optim_swap", table=bank.table.data_ptr(), n_seg=N, n_chunks=bank.n_chunks,      # noqa: E731
                                      grid_limit=grid_limit, stream=stream()))
    swap()
    torch.cuda.synchronize()
    once = bank.bits()
    for i, (o, n) in enumerate(zip(bank.offs, R.CASE_SIZES)):
        src = ("p", "ema") if i == R.CASE_NO_EMA else ("ema", "p")
        assert torch.equal(once["p"][o:o + n], before[src[0]][o:o + n]) and torch.equal(once["ema"][o:o + n], before[src[1]][o:o + n]), i
    assert bank.guards_intact()
    swap()
    torch.cuda.synchronize()
    for k, v in bank.bits().items():
        assert torch.equal(v, before[k]), k


def test_refusals_launch_nothing():
    bank = Bank()
    bank.upload_table()
    bank.put("g", R.case_grads(1))
    before, state = bank.bits(), bank.state.clone()
    base = dict(table=bank.table.data_ptr(), n_seg=N, n_chunks=bank.n_chunks, hyper=_hyper(R.CASE_MAX_NORM, 1),
                state=bank.state.data_ptr(), phase=0, scratch=bank.scratch.data_ptr(), scratch_bytes=bank.scratch.numel() * 8,
                grid_limit=0, stream=stream())
    for over, code in ((dict(table=None), hip.ERR_ARG), (dict(hyper=None), hip.ERR_ARG), (dict(state=None), hip.ERR_ARG),
                       (dict(scratch=None), hip.ERR_ARG), (dict(n_seg=0), hip.ERR_ARG), (dict(n_seg=70000), hip.ERR_ARG),
                       (dict(n_chunks=N - 1), hip.ERR_ARG), (dict(phase=-1), hip.ERR_ARG), (dict(grid_limit=-2), hip.ERR_ARG),
                       (dict(scratch_bytes=8 * bank.n_chunks - 8), hip.ERR_SIZE),
                       (dict(hyper=hip.OptimHyper(0.9, 1.0, 1e-8, 1.0, 0.5, 0, 0)), hip.ERR_ARG),
                       (dict(hyper=hip.OptimHyper(0.9, 0.999, float("nan"), 1.0, 0.5, 0, 0)), hip.ERR_ARG),
                       (dict(hyper=hip.OptimHyper(0.9, 0.999, 1e-8, float("nan"), 0.5, 0, 0)), hip.ERR_ARG),
                       (dict(hyper=hip.OptimHyper(0.9, 0.999, 1e-8, 1.0, -0.1, 0, 0)), hip.ERR_ARG)):
        assert hip.call("ditto_optim_adamw_step", **{**base, **over}) == code, over
        assert hip.lib().ditto_last_error()
    torch.cuda.synchronize()
    for k, v in bank.bits().items():
        assert torch.equal(v, before[k]), k
    assert torch.equal(bank.state, state)
