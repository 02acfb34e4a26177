"""-m gpu: the guided update that skips each utterance's speech prompt (csrc/guided_packed.hip) through its two entries,
ditto_guided_update_packed_prompt and ditto_guided_update_packed_tags_prompt.

Expected values come from the EXISTING entries run on the generated rows compacted into a packed batch of G_b-row utterances with the
same coefficients, seeds and tags: the generated rows must be torch.equal in both halves (the Philox index is local to the generated
region).  Prompt rows of x2 hold a sentinel pattern that must survive, those of eps2 hold NaN (they are not read).  Guard bands around
every buffer catch a write outside it."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8            # rows in front of and behind every buffer
# (d, rows per utterance, prompt rows per utterance): P = 0, G = 1, a one-row utterance; and one utterance whose quads (4200 x 256 / 4
# = 268800) exceed the 1024 x 256-lane grid, so that the grid stride wraps
SHAPES = {"small": (64, (5, 1, 9, 7), (0, 0, 8, 3)), "stride": (256, (4200,), (1,))}


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


class Case:
    """buffers of one call: x2 / eps2 [halves * S, d] and the noise [S, d], each inside guard bands"""

    def __init__(self, shape, cfg_on, noise):
        self.d, self.N, self.P = SHAPES[shape]
        d, N = self.d, self.N
        self.B, self.S, self.cfg_on, self.noise = len(N), sum(N), cfg_on, noise
        B, S = self.B, self.S
        self.cu = _cu(N)
        self.halves = 2 if cfg_on else 1
        x = hash_normal((S, d), "pu_x", 1)
        self.x = torch.cat([x] * self.halves).to(DEV)
        self.eps = hash_normal((self.halves * S, d), "pu_eps", 2).to(DEV)
        self.z = hash_normal((S, d), "pu_z", 3).to(DEV) if noise == "buffer" else None
        k = torch.arange(B, dtype=torch.float32)
        self.a, self.ce = (0.9 + 0.1 * k).to(DEV), (-0.2 + 0.15 * k).to(DEV)
        cz = 0.4 + 0.1 * k
        if B > 1:
            cz[1] = 0.0                                  # a sigma = 0 utterance among noisy ones (the tag form skips its draw)
        self.cz = cz.to(DEV)
        self.w = (2.0 + 0.5 * k).to(DEV) if cfg_on else None
        self.seeds = torch.tensor([5, -6, 2 ** 40 + 7, 8][:B], dtype=torch.int64, device=DEV) if noise == "philox" else None
        self.tags_l = [49, 17, 0xFFFFFFF0, 3][:B]
        self.tags = _i32([t - (1 << 32) if t >= 1 << 31 else t for t in self.tags_l])
        self.gen = torch.cat([torch.arange(self.cu[b] + self.P[b], self.cu[b + 1]) for b in range(B)]).to(DEV)
        is_p = torch.ones(S, dtype=torch.bool)
        is_p[self.gen.cpu()] = False
        self.prompt = torch.nonzero(is_p).reshape(-1).to(DEV)

    def guarded(self, t, fill=7.0):
        g = torch.full((GUARD, t.shape[1]), fill, dtype=t.dtype, device=DEV)
        pool = torch.cat([g, t, g]).contiguous()
        return pool, pool[GUARD:GUARD + t.shape[0]]

    def run(self, tag_form, x, eps, z, cu, prompt_len, B, S, max_N, step=49):
        """one of the four entries (prompt_len None: the existing ones), in place on x"""
        lib = hip.lib()
        head = (x.data_ptr(), eps.data_ptr(), _ptr(z), _ptr(self.seeds))
        tail = (_ptr(self.w), self.a.data_ptr(), self.ce.data_ptr(), self.cz.data_ptr(), cu.data_ptr())
        pl = () if prompt_len is None else (prompt_len.data_ptr(),)
        name = "ditto_guided_update_packed" + ("_tags" if tag_form else "") + ("" if prompt_len is None else "_prompt")
        hip.check(getattr(lib, name)(*head, self.tags.data_ptr() if tag_form else step, *tail, *pl, B, S, max_N, self.d,
                                     int(self.cfg_on), _s()))


@pytest.mark.parametrize("tag_form", [False, True], ids=["scalar_tag", "per_utt_tags"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("noise", ["philox", "none", "buffer"])
@pytest.mark.parametrize("shape", ["small", "stride"])
def test_prompted_update_equals_the_existing_kernel_on_the_compacted_rows(shape, noise, cfg_on, tag_form):
    c = Case(shape, cfg_on, noise)
    S, halves = c.S, c.halves
    G = [n - p for n, p in zip(c.N, c.P)]
    SG = sum(G)
    # expected: the existing entry over the generated rows alone
    gen2 = torch.cat([c.gen + h * S for h in range(halves)])
    want = c.x[gen2].contiguous()
    c.run(tag_form, want, c.eps[gen2].contiguous(), None if c.z is None else c.z[c.gen].contiguous(), _i32(_cu(G)), None, c.B, SG, max(G))
    # the prompted entry on the whole batch: sentinel prompt rows in x2, NaN prompt rows in eps2 (and in the noise buffer)
    x_in, eps_in = c.x.clone(), c.eps.clone()
    sent = (torch.arange(len(c.prompt) * c.d, dtype=torch.float32, device=DEV).reshape(-1, c.d) % 97) + 1000.0
    for h in range(halves):
        x_in[c.prompt + h * S] = sent
        eps_in[c.prompt + h * S] = float("nan")
    z_in = None
    if c.z is not None:
        z_in = c.z.clone()
        z_in[c.prompt] = float("nan")
    x_pool, x = c.guarded(x_in)
    eps_pool, eps = c.guarded(eps_in, float("nan"))
    c.run(tag_form, x, eps, z_in, _i32(c.cu), _i32(list(c.P)), c.B, S, max(c.N))
    assert torch.isfinite(want).all()
    assert torch.equal(x[gen2], want)
    for h in range(halves):
        assert torch.equal(x[c.prompt + h * S], sent), "a prompt row of x2 was written"
    assert torch.all(x_pool[:GUARD] == 7.0) and torch.all(x_pool[-GUARD:] == 7.0)
    if noise == "philox" and shape == "small":       # the draw is local to the generated region: it is not the whole-utterance draw
        plain = c.x.clone()
        c.run(tag_form, plain, c.eps, None, _i32(c.cu), None, c.B, S, max(c.N))
        lo = c.cu[2] + c.P[2]
        assert not torch.equal(plain[lo:c.cu[3]], x[lo:c.cu[3]])


@pytest.mark.parametrize("tag_form", [False, True], ids=["scalar_tag", "per_utt_tags"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("noise", ["philox", "none", "buffer"])
def test_prompt_len_all_zero_is_the_existing_entry(noise, cfg_on, tag_form):
    c = Case("small", cfg_on, noise)
    want, got = c.x.clone(), c.x.clone()
    c.run(tag_form, want, c.eps, c.z, _i32(c.cu), None, c.B, c.S, max(c.N))
    c.run(tag_form, got, c.eps, c.z, _i32(c.cu), _i32([0] * c.B), c.B, c.S, max(c.N))
    assert torch.isfinite(want).all() and torch.equal(got, want)


@pytest.mark.parametrize("tag_form", [False, True], ids=["scalar_tag", "per_utt_tags"])
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_bad_prompt_len_is_clamped_into_the_utterance(cfg_on, tag_form):
    """prompt_len[b] = -3 acts as 0 and N_b + 5 as N_b - 1: wrong rows at worst, nothing outside the utterance's own rows and nothing
    outside the buffer"""
    c = Case("small", cfg_on, "philox")
    S, halves = c.S, c.halves
    bad = [-3, c.N[1] + 5, c.N[2] + 5, -3]
    clamped = [0, c.N[1] - 1, c.N[2] - 1, 0]
    want = c.x.clone()
    c.run(tag_form, want, c.eps, None, _i32(c.cu), _i32(clamped), c.B, S, max(c.N))
    x_pool, x = c.guarded(c.x)
    eps_pool, eps = c.guarded(c.eps, float("nan"))
    c.run(tag_form, x, eps, None, _i32(c.cu), _i32(bad), c.B, S, max(c.N))
    assert torch.isfinite(want).all() and torch.equal(x, want)
    assert torch.all(x_pool[:GUARD] == 7.0) and torch.all(x_pool[-GUARD:] == 7.0)
    for h in range(halves):                              # utterance 2 kept all but its last row
        lo = h * S + c.cu[2]
        assert torch.equal(x[lo:lo + c.N[2] - 1], c.x[lo:lo + c.N[2] - 1])
