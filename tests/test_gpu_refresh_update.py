"""-m gpu: the three-kind update of a refresh stream (csrc/guided_refresh.hip, ditto_guided_update_packed_refresh) at kernel level.

One launch holds refreshing, reusing and plain utterances.  Expected values come from the EXISTING entries on the same inputs:
ditto_guided_update_packed_mixed gives the refreshing utterances (both copies) and the plain ones, bit for bit;
ditto_guided_update_packed_reuse in LOAD mode, called once per distinct tag, gives the reusing ones (a scalar-tag kernel: the compared
utterances have cz != 0); torch's fp32 c - u gives the kept direction.  d = 64 and 256, lengths (1, 3, 17, 64, 5) — a one-row
utterance, odd lengths and one of several workgroups — with prompts on some.  Prompt rows of x2 hold a sentinel that must survive,
those of eps2, delta and the noise buffer hold NaN (they are not read); NaN guard rows stand around every buffer and must keep their
bits, and a read from them would show as NaN in the result."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
N = [1, 3, 17, 64, 5]
P = [0, 1, 5, 0, 2]
PLAIN, REFRESH, REUSE = hip.KIND_PLAIN, hip.KIND_REFRESH, hip.KIND_REUSE
KIND = [REUSE, REFRESH, PLAIN, REFRESH, REUSE]
PARTNER = [-1, 0, -1, 1, -1]
B, S = len(N), sum(N)
TAGS = [49, 17, 3, 0xFFFFFFF0, 49]             # the two reusing utterances share a tag with nobody / with each other: 49 twice
NOISES = ["philox", "none", "buffer"]
DS = [64, 256]
UPDATE = "ditto_guided_update_packed_refresh"


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
    return torch.tensor([x - (1 << 32) if x >= 1 << 31 else x for x in v], dtype=torch.int32, device=DEV)


CU = _cu(N)


def _rows(b, lo=0):
    return torch.arange(CU[b] + lo, CU[b + 1], device=DEV)


def _guarded(t):
    g = torch.full((GUARD, t.shape[1]), float("nan"), dtype=t.dtype, device=DEV)
    pool = torch.cat([g, t, g]).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module", params=DS, ids=[f"d{d}" for d in DS])
def data(request):
    """the inputs every test of one width shares (read-only)"""
    d = request.param
    k = torch.arange(B, dtype=torch.float32)
    return dict(d=d, x=hash_normal((S, d), "rf_x", 1).to(DEV), eps_c=hash_normal((S, d), "rf_eps", 2).to(DEV),
                eps_u=hash_normal((S, d), "rf_eps", 3).to(DEV), z=hash_normal((S, d), "rf_z", 4).to(DEV),
                delta=hash_normal((S, d), "rf_delta", 5).to(DEV), a=(0.9 + 0.1 * k).to(DEV), ce=(-0.2 + 0.15 * k).to(DEV),
                # cz != 0 on the reusing utterances (0 and 4), compared with a scalar-tag kernel; a sigma = 0 utterance among the
                # refreshing and among the plain ones: no draw there, as in the mixed kernel
                cz=torch.tensor([0.25, 0.0, 0.0, 0.4, 0.3], device=DEV), w=(2.0 + 0.5 * k).to(DEV),
                seeds=torch.tensor([5, -6, 2 ** 40 + 7, 8, -9], dtype=torch.int64, device=DEV), tags=_i32(TAGS))


class Call:
    """one call over the mixed layout: x2 / eps2 [S + S_G, d] and delta / noise [S, d] with sentinel / NaN prompt rows, inside NaN
    guards.  entry "refresh": the new one; "mixed": ditto_guided_update_packed_mixed on the same buffers (no kind, no delta)"""

    def __init__(self, dt, noise, kind, partner, entry="refresh", G=None, w=None, prompts=P):
        d = dt["d"]
        self.guided = [b for b in range(B) if partner[b] >= 0] if G is None else G
        g = self.guided
        self.cu_g = _cu([N[b] for b in g])
        self.S_G = self.cu_g[-1]
        x = torch.cat([dt["x"]] + [dt["x"][_rows(b)] for b in g])
        eps = torch.cat([dt["eps_c"]] + [dt["eps_u"][_rows(b)] for b in g])
        z = dt["z"].clone() if noise == "buffer" else None
        delta = dt["delta"].clone()
        self.prompt_rows, self.own_prompt_rows = [], []
        for b in range(B):
            if not prompts[b]:
                continue
            at = [CU[b]] + ([S + self.cu_g[g.index(b)]] if b in g else [])
            for lo in at:
                r = torch.arange(lo, lo + prompts[b], device=DEV)
                self.prompt_rows.append(r)
                x[r] = (torch.arange(len(r) * d, dtype=torch.float32, device=DEV).reshape(-1, d) % 97) + 1000.0
                eps[r] = float("nan")
            own = torch.arange(CU[b], CU[b] + prompts[b], device=DEV)
            self.own_prompt_rows.append(own)
            delta[own] = float("nan")
            if z is not None:
                z[own] = float("nan")
        self.x_pool, self.x = _guarded(x)
        self.eps_pool, self.eps = _guarded(eps)
        self.z_pool, self.z = _guarded(z) if z is not None else (None, None)
        self.delta_pool, self.delta = _guarded(delta)
        self.x_before, self.delta_before = self.x_pool.clone(), self.delta_pool.clone()
        offsets, part = _i32(CU + [S + c for c in self.cu_g[1:]]), _i32(partner)
        pld, kd = _i32(prompts), None if kind is None else _i32(kind)
        w = dt["w"] if w is None else w
        common = dict(x2=self.x.data_ptr(), eps2=self.eps.data_ptr(), noise=_ptr(self.z), seeds=_ptr(dt["seeds"]) if noise == "philox" else None,
                      tags=dt["tags"].data_ptr(), w=w.data_ptr(), a=dt["a"].data_ptr(), ce=dt["ce"].data_ptr(), cz=dt["cz"].data_ptr(),
                      cu=offsets.data_ptr(), partner=part.data_ptr(), prompt_len=pld.data_ptr(), B=B, G=len(g), S=S, S_G=self.S_G,
                      max_N=max(N), d=d, stream=_s())
        if entry == "refresh":
            hip.check(hip.call(UPDATE, **common, delta=self.delta.data_ptr(), kind=kd.data_ptr()))
        else:
            hip.check(hip.call("ditto_guided_update_packed_mixed", **common))
        torch.cuda.synchronize()

    def copy_rows(self, b, lo=0):
        k = self.guided.index(b)
        return torch.arange(S + self.cu_g[k] + lo, S + self.cu_g[k + 1], device=DEV)

    def check_guards(self):
        for pool, before in ((self.x_pool, self.x_before), (self.delta_pool, self.delta_before)):
            assert _same_bits(pool[:GUARD], before[:GUARD]) and _same_bits(pool[-GUARD:], before[-GUARD:])
            assert torch.isnan(pool[:GUARD]).all() and torch.isnan(pool[-GUARD:]).all()

    def check_untouched(self):
        for r in self.prompt_rows:
            assert _same_bits(self.x[r], self.x_before[GUARD:][r]), "a prompt row of x2 was written"
        for r in self.own_prompt_rows:
            assert _same_bits(self.delta[r], self.delta_before[GUARD:][r]), "a prompt row of delta was written"
        self.check_guards()


def _reuse_load(dt, noise, tag, w=None):
    """ditto_guided_update_packed_reuse in LOAD mode over the B utterances with the scalar tag `tag`: x' [S, d]"""
    d = dt["d"]
    x = dt["x"].clone()
    delta = dt["delta"].clone()
    z = dt["z"].clone() if noise == "buffer" else None
    cu, pld = _i32(CU), _i32(P)
    w = dt["w"] if w is None else w
    hip.check(hip.call("ditto_guided_update_packed_reuse", x2=x.data_ptr(), eps=dt["eps_c"].data_ptr(), delta=delta.data_ptr(), noise=_ptr(z),
                       seeds=_ptr(dt["seeds"]) if noise == "philox" else None, step=tag, w=w.data_ptr(), a=dt["a"].data_ptr(),
                       ce=dt["ce"].data_ptr(), cz=dt["cz"].data_ptr(), cu=cu.data_ptr(), prompt_len=pld.data_ptr(), suffix_len=None, B=B, S=S,
                       max_N=max(N), d=d, mode=hip.REUSE_LOAD, mirror=0, stream=_s()))
    torch.cuda.synchronize()
    assert _same_bits(delta, dt["delta"])
    return x


@pytest.mark.parametrize("noise", NOISES)
def test_refresh_and_plain_rows_are_the_mixed_kernels_and_reuse_rows_the_reuse_kernels(data, noise):
    m = Call(data, noise, KIND, PARTNER)
    want = Call(data, noise, None, PARTNER, entry="mixed")
    before = m.x_before[GUARD:GUARD + S + m.S_G]
    for b in (1, 3):                                                    # refresh: both copies, and the direction kept
        own, cp = _rows(b, P[b]), m.copy_rows(b, P[b])
        assert torch.isfinite(m.x[own]).all() and not torch.equal(m.x[own], before[own])
        assert _same_bits(m.x[own], want.x[own]), f"utterance {b}, its own rows"
        assert _same_bits(m.x[cp], want.x[cp]) and _same_bits(m.x[cp], m.x[own]), f"utterance {b}, the copy"
        assert _same_bits(m.delta[own], data["eps_c"][own] - data["eps_u"][own]), f"utterance {b}, delta"
    assert _same_bits(m.x[_rows(2, P[2])], want.x[_rows(2, P[2])]), "the plain utterance"
    for tag in sorted({TAGS[b] for b in (0, 4)}):                       # reuse: the LOAD kernel, per distinct tag
        load = _reuse_load(data, noise, tag)
        for b in (0, 4):
            if TAGS[b] == tag:
                own = _rows(b, P[b])
                assert torch.isfinite(m.x[own]).all()
                assert _same_bits(m.x[own], load[own]), f"utterance {b}, reuse"
                assert not torch.equal(m.x[own], want.x[own])             # the direction matters (mixed ran it without guidance)
    # delta: reuse and plain utterances, prompt rows and guards keep their bits; nothing behind row S but the refresh copies changed
    for b in (0, 2, 4):
        assert _same_bits(m.delta[_rows(b)], m.delta_before[GUARD:][_rows(b)]), f"delta of utterance {b} was written"
    m.check_untouched()
    assert torch.isfinite(m.x[torch.cat([_rows(b, P[b]) for b in range(B)])]).all()


@pytest.mark.parametrize("noise", NOISES)
def test_unit_scale_makes_reuse_equal_plain(data, noise):
    one = torch.ones(B, device=DEV)
    reuse = Call(data, noise, [REUSE] * B, [-1] * B, w=one)
    plain = Call(data, noise, [PLAIN] * B, [-1] * B, w=one)
    assert reuse.S_G == 0 and reuse.x.shape[0] == S
    gen = torch.cat([_rows(b, P[b]) for b in range(B)])
    assert torch.isfinite(plain.x[gen]).all() and _same_bits(reuse.x, plain.x)
    assert not torch.equal(plain.x[gen], plain.x_before[GUARD:][gen])
    for c in (reuse, plain):
        assert _same_bits(c.delta_pool, c.delta_before)                  # neither wrote a direction
        c.check_untouched()
    mixed = Call(data, noise, None, [-1] * B, entry="mixed", w=one)
    assert _same_bits(plain.x, mixed.x)


@pytest.mark.parametrize("noise", NOISES)
def test_everyone_refreshing_is_the_mixed_kernel_with_the_identity_partner(data, noise):
    m = Call(data, noise, [REFRESH] * B, list(range(B)))
    want = Call(data, noise, None, list(range(B)), entry="mixed")
    assert m.S_G == S and _same_bits(m.x, want.x)
    for b in range(B):
        own = _rows(b, P[b])
        assert _same_bits(m.delta[own], data["eps_c"][own] - data["eps_u"][own])
    m.check_untouched()


@pytest.mark.parametrize("noise", NOISES)
def test_out_of_range_kinds_and_partners_touch_nothing_outside_the_buffers(data, noise):
    """kind outside 0..2 counts as plain, a refresh without a usable partner too; the partner is clamped into [-1, G - 1] and the
    copy's span into [S, S + S_G): wrong rows, never an access outside x2 [S + S_G, d] or delta [S, d]"""
    none = [0] * B
    m = Call(data, noise, [7, -3, REFRESH, REFRESH, 2 ** 31 - 1], [5, -7, -2, 2 ** 31 - 1, 0], G=[1, 3], prompts=none)
    m.check_guards()
    assert torch.isfinite(m.x).all()                                     # NaN stands in the guards only
    before = m.x_before[GUARD:GUARD + S + m.S_G]
    plain = Call(data, noise, [PLAIN] * B, [-1] * B, prompts=none)
    for b in (0, 1, 2, 4):                                               # bad kinds, and a refresh whose partner is negative: plain
        assert _same_bits(m.x[_rows(b)], plain.x[_rows(b)]), b
        assert _same_bits(m.delta[_rows(b)], m.delta_before[GUARD:][_rows(b)]), b
    assert not torch.equal(m.x[_rows(3)], plain.x[_rows(3)])             # 2^31 - 1 -> copy 1, its own: a refresh
    assert _same_bits(m.x[m.copy_rows(1)], before[m.copy_rows(1)])       # copy 0, which no usable partner names, is not written
    # a refresh longer than all the copies has no copy: plain, and its direction is not written
    m = Call(data, noise, [REFRESH] * B, [0] * B, G=[0], prompts=none)
    assert m.S_G == 1
    m.check_guards()
    for b in (1, 2, 3, 4):
        assert _same_bits(m.x[_rows(b)], plain.x[_rows(b)]) and _same_bits(m.delta[_rows(b)], m.delta_before[GUARD:][_rows(b)])
    assert _same_bits(m.delta[_rows(0)], data["eps_c"][_rows(0)] - data["eps_u"][_rows(0)])
