"""-m gpu: the guided update over a window per utterance (csrc/guided_packed.hip: speech infilling) through its two entries,
ditto_guided_update_packed_window and ditto_guided_update_packed_tags_window.

Expected values come from the EXISTING unprompted entries run on the window rows compacted into a packed batch of G_b-row utterances
with the same coefficients, seeds and tags: the window rows must be torch.equal in both halves (the Philox index is local to the
window).  Context rows of x2, on both sides, hold a sentinel pattern that must survive; those of eps2 and of a noise buffer hold NaN
(they are not read).  Guard bands around every buffer catch a write outside it.  With every Q_b = 0 the whole x2 is the _prompt
entry's.  The clamp case uses the bad (P, Q) values of tests/test_window_host.py and its restated clamp."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal
from test_window_host import BAD_WINDOWS, window_clamp

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8            # rows in front of and behind every buffer
# d, then (rows, prefix rows, suffix rows) per utterance: no context, a one-row utterance, a prefix only with G = 1, G = 1 between two
# contexts, a suffix only, both; and one utterance whose window quads (4200 x 256 / 4 = 268800) exceed the 1024 x 256-lane grid, so that
# the grid stride wraps
SHAPES = {"small": (64, ((5, 0, 0), (1, 0, 0), (9, 8, 0), (7, 3, 3), (6, 0, 4), (12, 2, 3))), "stride": (256, ((4202, 1, 1),))}


def _ptr(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def window_rows(cu, P, Q):
    """(rows of every utterance's window, the other rows), as device index tensors"""
    S = cu[-1]
    gen = torch.cat([torch.arange(cu[b] + P[b], cu[b + 1] - Q[b]) for b in range(len(P))])
    is_c = torch.ones(S, dtype=torch.bool)
    is_c[gen] = False
    return gen.to(DEV), torch.nonzero(is_c).reshape(-1).to(DEV)


class Case:
    """buffers of one call: x2 / eps2 [halves * S, d] and the noise [S, d]"""

    def __init__(self, shape, cfg_on, noise):
        self.d, npq = SHAPES[shape]
        self.N, self.P, self.Q = ([v[i] for v in npq] for i in range(3))
        d, N = self.d, self.N
        self.B, self.S, self.cfg_on, self.noise = len(N), sum(N), cfg_on, noise
        B, S = self.B, self.S
        self.cu = _cu(N)
        self.halves = 2 if cfg_on else 1
        x = hash_normal((S, d), "wu_x", 1)
        self.x = torch.cat([x] * self.halves).to(DEV)
        self.eps = hash_normal((self.halves * S, d), "wu_eps", 2).to(DEV)
        self.z = hash_normal((S, d), "wu_z", 3).to(DEV) if noise == "buffer" else None
        k = torch.arange(B, dtype=torch.float32)
        self.a, self.ce = (0.9 + 0.1 * k).to(DEV), (-0.2 + 0.15 * k).to(DEV)
        cz = 0.4 + 0.1 * k
        if B > 1:
            cz[3] = 0.0                                  # a sigma = 0 utterance among noisy ones (the tag form skips its draw)
        self.cz = cz.to(DEV)
        self.w = (2.0 + 0.5 * k).to(DEV) if cfg_on else None
        self.seeds = torch.tensor([5, -6, 2 ** 40 + 7, 8, -(2 ** 33) - 1, 11][:B], dtype=torch.int64, device=DEV) if noise == "philox" else None
        self.tags_l = [49, 17, 0xFFFFFFF0, 3, 0, 24][:B]
        self.tags = _i32([t - (1 << 32) if t >= 1 << 31 else t for t in self.tags_l])
        self.gen, self.ctx = window_rows(self.cu, self.P, self.Q)

    def guarded(self, t, fill=7.0):
        g = torch.full((GUARD, t.shape[1]), fill, dtype=t.dtype, device=DEV)
        pool = torch.cat([g, t, g]).contiguous()
        return pool, pool[GUARD:GUARD + t.shape[0]]

    def run(self, tag_form, x, eps, z, cu, prompt_len, suffix_len, B, S, max_N, step=49, null_prompt=False):
        """one of the six entries (suffix_len None: the _prompt ones; prompt_len None too: the unprompted ones), in place on x"""
        lib = hip.lib()
        head = (x.data_ptr(), eps.data_ptr(), _ptr(z), _ptr(self.seeds))
        tail = (_ptr(self.w), self.a.data_ptr(), self.ce.data_ptr(), self.cz.data_ptr(), cu.data_ptr())
        if suffix_len is not None:
            ctx, kind = (None if null_prompt else prompt_len.data_ptr(), suffix_len.data_ptr()), "_window"
        elif prompt_len is not None:
            ctx, kind = (prompt_len.data_ptr(),), "_prompt"
        else:
            ctx, kind = (), ""
        name = "ditto_guided_update_packed" + ("_tags" if tag_form else "") + kind
        hip.check(getattr(lib, name)(*head, self.tags.data_ptr() if tag_form else step, *tail, *ctx, B, S, max_N, self.d,
                                     int(self.cfg_on), _s()))


def _guards_intact(*pools):
    for pool, fill in pools:
        for band in (pool[:GUARD], pool[-GUARD:]):
            if fill != fill:
                assert torch.isnan(band).all()
            else:
                assert torch.all(band == fill)


@pytest.mark.parametrize("tag_form", [False, True], ids=["scalar_tag", "per_utt_tags"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("noise", ["philox", "none", "buffer"])
@pytest.mark.parametrize("shape", ["small", "stride"])
def test_windowed_update_equals_the_existing_kernel_on_the_compacted_rows(shape, noise, cfg_on, tag_form):
    c = Case(shape, cfg_on, noise)
    S, halves = c.S, c.halves
    G = [n - p - q for n, p, q in zip(c.N, c.P, c.Q)]
    SG = sum(G)
    # expected: the existing unprompted entry over the window rows alone
    gen2 = torch.cat([c.gen + h * S for h in range(halves)])
    want = c.x[gen2].contiguous()
    c.run(tag_form, want, c.eps[gen2].contiguous(), None if c.z is None else c.z[c.gen].contiguous(), _i32(_cu(G)), None, None, c.B, SG,
          max(G))
    # the windowed entry on the whole batch: sentinel context rows in x2, NaN context rows in eps2 (and in the noise buffer)
    x_in, eps_in = c.x.clone(), c.eps.clone()
    sent = (torch.arange(len(c.ctx) * c.d, dtype=torch.float32, device=DEV).reshape(-1, c.d) % 97) + 1000.0
    for h in range(halves):
        x_in[c.ctx + h * S] = sent
        eps_in[c.ctx + h * S] = float("nan")
    x_pool, x = c.guarded(x_in)
    eps_pool, eps = c.guarded(eps_in, float("nan"))
    z_pool = z = None
    if c.z is not None:
        z_in = c.z.clone()
        z_in[c.ctx] = float("nan")
        z_pool, z = c.guarded(z_in, float("nan"))
    eps_before = eps_pool.clone()
    c.run(tag_form, x, eps, z, _i32(c.cu), _i32(c.P), _i32(c.Q), c.B, S, max(c.N))
    assert torch.isfinite(want).all()
    assert torch.equal(x[gen2], want)
    for h in range(halves):
        assert torch.equal(x[c.ctx + h * S], sent), "a context row of x2 was written"
    _guards_intact((x_pool, 7.0), (eps_pool, float("nan")), *(() if z_pool is None else ((z_pool, float("nan")),)))
    assert torch.equal(eps_pool.view(torch.int32), eps_before.view(torch.int32)), "eps2 was written"
    if noise == "philox" and shape == "small":       # the draw is local to the window: it is not the whole-utterance draw
        plain = c.x.clone()
        c.run(tag_form, plain, c.eps, None, _i32(c.cu), None, None, c.B, S, max(c.N))
        lo, hi = c.cu[5] + c.P[5], c.cu[6] - c.Q[5]
        assert not torch.equal(plain[lo:hi], x[lo:hi])


@pytest.mark.parametrize("null_prompt", [False, True], ids=["prompt_len", "null_prompt_len"])
@pytest.mark.parametrize("tag_form", [False, True], ids=["scalar_tag", "per_utt_tags"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("noise", ["philox", "none", "buffer"])
def test_suffix_len_all_zero_is_the_prompt_entry(noise, cfg_on, tag_form, null_prompt):
    """Q_b = 0 for every b: the whole x2 is the _prompt entry's; with a NULL prompt_len as well, the _prompt entry's with P all 0"""
    c = Case("small", cfg_on, noise)
    P = [0] * c.B if null_prompt else c.P
    want, got = c.x.clone(), c.x.clone()
    c.run(tag_form, want, c.eps, c.z, _i32(c.cu), _i32(P), None, c.B, c.S, max(c.N))
    c.run(tag_form, got, c.eps, c.z, _i32(c.cu), _i32(P), _i32([0] * c.B), c.B, c.S, max(c.N), null_prompt=null_prompt)
    assert torch.isfinite(want).all() and torch.equal(got, want)


def test_null_suffix_len_is_refused():
    c = Case("small", True, "none")
    x = c.x.clone()
    for name, tag in (("ditto_guided_update_packed_window", 49), ("ditto_guided_update_packed_tags_window", c.tags.data_ptr())):
        rc = getattr(hip.lib(), name)(x.data_ptr(), c.eps.data_ptr(), None, None, tag, c.w.data_ptr(), c.a.data_ptr(), c.ce.data_ptr(),
                                      c.cz.data_ptr(), _i32(c.cu).data_ptr(), None, None, c.B, c.S, max(c.N), c.d, 1, _s())
        assert rc == hip.ERR_ARG
    assert torch.equal(x, c.x)


@pytest.mark.parametrize("tag_form", [False, True], ids=["scalar_tag", "per_utt_tags"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_bad_context_lengths_are_clamped_into_the_utterance(cfg_on, tag_form):
    """negative, too large and P + Q >= n values: the rows written are those the restated clamp (tests/test_window_host.py) predicts,
    nothing outside the utterance's own rows and nothing outside the buffers"""
    c = Case("small", cfg_on, "philox")
    S, halves = c.S, c.halves
    bad = [BAD_WINDOWS[b % len(BAD_WINDOWS)] for b in range(c.B)]
    good = [window_clamp(c.N[b], *bad[b]) for b in range(c.B)]
    assert any(g != tuple(v) for g, v in zip(good, bad))
    want = c.x.clone()
    c.run(tag_form, want, c.eps, None, _i32(c.cu), _i32([g[0] for g in good]), _i32([g[1] for g in good]), c.B, S, max(c.N))
    x_pool, x = c.guarded(c.x)
    eps_pool, eps = c.guarded(c.eps, float("nan"))
    c.run(tag_form, x, eps, None, _i32(c.cu), _i32([v[0] for v in bad]), _i32([v[1] for v in bad]), c.B, S, max(c.N))
    assert torch.isfinite(want).all() and torch.equal(x, want)
    _guards_intact((x_pool, 7.0), (eps_pool, float("nan")))
    gen, ctx = window_rows(c.cu, [g[0] for g in good], [g[1] for g in good])
    for h in range(halves):                              # exactly the predicted rows moved
        assert torch.equal(x[ctx + h * S], c.x[ctx + h * S])
        assert not (x[gen + h * S] == c.x[gen + h * S]).all(dim=1).any()
