"""-m gpu: the guidance-rescale statistics (csrc/guided_rescale.hip) through ditto_guidance_rescale_packed.

Every utterance's scale and coef_out are held to the DERIVED bound of tests/rescale_ref.py against its fp64 reference — no utterance
is exempt — at d = 64, 256 and 768, over generated regions of one row, exactly one chunk of 4096 quads (d = 768: 64 rows, exactly three
— no whole number of 768-wide rows makes one), one chunk plus one row and several chunks, each with and without a prompt (P_b = n_b - 1
among them), in the doubled and in the mixed layout (some partner = -1, gaps between the copies), for coefficient arrays and for
ditto_multistep_coef [B].  Then what must be EXACT: phi = 0 and unguided utterances are bit copies with scale 1.0; all-zero eps gives
1.0; NaN in every row the contract says is not read changes nothing; the guard bands around eps2 and the scratch and the unused bytes
of the scratch survive; the same utterance somewhere else, among other neighbours, in a batch of another B, with max_N exact or
under-reported, gets the same bits; two runs agree; out-of-range prompt lengths, partners and offsets behave as their clamped values.
No case here reaches outside a buffer: the clamps are checked by their results, inside the guards."""
import functools

import numpy as np
import pytest
import torch

import rescale_ref as R
from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_ROWS, GUARD_BYTES, FILL = 4, 512, 0xA5
CHUNK = hip.RESCALE_CHUNK_QUADS * 4                      # elements of one partial
WS, PHIS = (5.0, 0.0, 2.5, 1.0), (1.0, 0.7, 0.0, 0.3)


def _utterances(d):
    """(key, generated rows, prompt rows): the regions of the module docstring"""
    one = CHUNK // d if CHUNK % d == 0 else 3 * CHUNK // d      # rows of exactly one chunk (d = 768: of exactly three)
    part = (CHUNK // d + 1) if CHUNK % d else one + 1            # one chunk plus (a part of) one row
    return [(0, 1, 0), (1, 1, 7), (2, one, 0), (3, one, 3), (4, part, 0), (5, one + 1, 5), (6, 3 * one + 5, 0), (7, 2 * one + 9, 2)]


@functools.lru_cache(maxsize=None)
def _eps(key, n, d):
    """utterance `key`'s conditional and unconditional eps [n, d], a function of the utterance alone (correlated, as the halves are)"""
    c = hash_normal((n, d), "rs_c", key)
    return c, (0.8 * c + 0.6 * hash_normal((n, d), "rs_u", key)).contiguous()


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


class Batch:
    """a packed batch of utterances [(key, g, p)] with per-utterance w and phi; `guided` (mixed layout): who has a copy"""

    def __init__(self, d, utts, ws, phis, guided=None):
        self.d, self.utts, self.B = d, utts, len(utts)
        self.n = [g + p for _, g, p in utts]
        self.p = [p for _, _, p in utts]
        self.cu, self.S = _cu(self.n), sum(self.n)
        self.w, self.phi = list(ws), list(phis)
        self.guided = guided
        self.eps = [_eps(k, n, d) for (k, _, _), n in zip(utts, self.n)]
        self.coef_in = [(-1.0) ** b * (0.05 + 0.11 * b) for b in range(self.B)]
        if guided is None:
            self.partner, self.G, self.S_G, self.ucu = None, 0, 0, None
            self.offsets = self.cu + [self.S + c for c in self.cu[1:]]
        else:                                             # copies behind the S rows, one unread gap row behind each where S_G <= S allows
            self.partner, g, at, self.ucu = [], 0, 0, []
            gap = int(sum(n for n, f in zip(self.n, guided) if not f) >= sum(guided))
            for b in range(self.B):
                self.partner.append(g if guided[b] else -1)
                if guided[b]:
                    self.ucu.append(at)
                    at += self.n[b] + gap
                    g += 1
            self.G, self.S_G = g, at
            self.offsets = self.cu[:-1] + [self.S] + [self.S + u for u in self.ucu[1:]] + ([self.S + at] if g else [])

    def active(self, b):
        return (self.guided is None or self.guided[b]) and min(max(np.float32(self.phi[b]), 0), 1) > 0

    def eps2(self, nan, zero=False):
        """(pool with NaN guard rows, the view the library gets).  nan: NaN in every row the contract says is not read — prompt rows,
        all rows of an utterance that is not rescaled (phi == 0 or no partner), the gap rows behind the copies"""
        rows = 2 * self.S if self.guided is None else self.S + self.S_G
        t = torch.full((rows, self.d), float("nan") if nan else 0.25)
        for b in range(self.B):
            c, u = (x.clone() for x in self.eps[b])
            if nan:
                c[:self.p[b]] = float("nan")
                u[:self.p[b]] = float("nan")
                if not self.active(b):
                    c[:], u[:] = float("nan"), float("nan")
            t[self.cu[b]:self.cu[b + 1]] = c
            if self.guided is None:
                t[self.S + self.cu[b]:self.S + self.cu[b + 1]] = u
            elif self.guided[b]:
                at = self.S + self.ucu[self.partner[b]]
                t[at:at + self.n[b]] = u
        if zero:
            t.zero_()
        g = torch.full((GUARD_ROWS, self.d), float("nan"))
        pool = torch.cat([g, t, g]).to(DEV).contiguous()
        return pool, pool[GUARD_ROWS:GUARD_ROWS + rows]

    def reference(self):
        """[(s fp64, bound on s32, bound on coef_out per |coef_in|)] per utterance, from the generated rows alone"""
        out = []
        for b in range(self.B):
            c, u = (x[self.p[b]:].numpy() for x in self.eps[b])
            guided = self.guided is None or self.guided[b]
            out.append((R.reference(c, u, self.w[b], self.phi[b], guided)["s"], *R.bound(c, u, self.w[b], self.phi[b], guided)))
        return out


def run(bt, form="array", nan=False, zero=False, max_N=None, offsets=None, prompt=None, partner=None, with_prompt=True):
    """one call -> (scale [B], coef_out [B] or [B, 8], coef_in likewise) on the CPU; asserts the guards and unused bytes survived"""
    lib, B = hip.lib(), bt.B
    true_max = max(g for _, g, _ in bt.utts)
    need = lib.ditto_guidance_rescale_bytes(B, true_max, bt.d)
    assert need > 0
    pool = torch.full((need + 2 * GUARD_BYTES,), FILL, dtype=torch.uint8, device=DEV)
    scratch = pool[GUARD_BYTES:GUARD_BYTES + need]
    assert scratch.data_ptr() % 256 == 0
    epool, eps2 = bt.eps2(nan, zero)
    ebits = epool.view(torch.int32).clone()
    phi = torch.tensor(bt.phi, dtype=torch.float32, device=DEV)
    w = torch.tensor(bt.w, dtype=torch.float32, device=DEV)
    cin = torch.tensor(bt.coef_in, dtype=torch.float32, device=DEV)
    if form == "struct":                                  # a, kx, ke, b, g, w | use_prev | reserved
        co = hash_normal((B, 8), "rs_coef", 1).to(DEV).contiguous()
        co[:, 2], co[:, 5] = cin, w
        co.view(torch.int32)[:, 6] = torch.arange(B, device=DEV, dtype=torch.int32) % 2
        co.view(torch.int32)[:, 7] = 0
        args_c = (None, phi.data_ptr(), None, co.data_ptr())
        cin_full = co
    else:
        args_c = (w.data_ptr(), phi.data_ptr(), cin.data_ptr(), None)
        cin_full = cin
    off = _i32(bt.offsets if offsets is None else offsets)
    pl = _i32(bt.p if prompt is None else prompt) if with_prompt else None
    pt = None if bt.partner is None else _i32(bt.partner if partner is None else partner)
    hip.check(lib.ditto_guidance_rescale_packed(
        eps2.data_ptr(), *args_c, off.data_ptr(), None if pl is None else pl.data_ptr(), None if pt is None else pt.data_ptr(), B, bt.G,
        bt.S, bt.S_G, true_max if max_N is None else max_N, bt.d, scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    o_scale, o_part = hip.rescale_scratch_layout(B)
    nout = 32 * B if form == "struct" else 4 * B
    host = pool.cpu()
    assert (host[:GUARD_BYTES] == FILL).all() and (host[GUARD_BYTES + need:] == FILL).all(), "a guard band of the scratch was written"
    sc = host[GUARD_BYTES:GUARD_BYTES + need]
    assert (sc[nout:o_scale] == FILL).all() and (sc[o_scale + 4 * B:o_part] == FILL).all(), "unused bytes of the scratch were written"
    assert torch.equal(epool.view(torch.int32), ebits), "eps2 or its guard rows were written"
    out = sc[:nout].clone().view(torch.float32)
    return sc[o_scale:o_scale + 4 * B].clone().view(torch.float32), out.view(B, 8) if form == "struct" else out, cin_full.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _batch(d, layout):
    utts = _utterances(d)
    B = len(utts)
    ws, phis = [WS[b % 4] for b in range(B)], [PHIS[(b + b // 4) % 4] for b in range(B)]
    guided = None if layout == "doubled" else [b not in (1, 6) for b in range(B)]     # (so: unguided with phi > 0, guided with phi == 0)
    return Batch(d, utts, ws, phis, guided)


@pytest.fixture(scope="module")
def cases():
    """batch and reference per (d, layout): built and computed once"""
    memo = {}

    def get(d, layout):
        if (d, layout) not in memo:
            bt = _batch(d, layout)
            memo[d, layout] = (bt, bt.reference())
        return memo[d, layout]
    return get


@pytest.mark.parametrize("form", ["array", "struct"])
@pytest.mark.parametrize("layout", ["doubled", "mixed"])
@pytest.mark.parametrize("d", [64, 256, 768])
def test_scale_and_coef_inside_the_derived_bound_and_exact_cases(cases, d, layout, form):
    bt, ref = cases(d, layout)
    scale, out, cin = run(bt, form)
    assert sum(bt.active(b) for b in range(bt.B)) >= 4 and not all(bt.active(b) for b in range(bt.B))
    k_in = cin[:, 2] if form == "struct" else cin
    k_out = out[:, 2] if form == "struct" else out
    for b in range(bt.B):
        s, bs, bc = ref[b]
        err_s, err_c = abs(float(scale[b]) - s), abs(float(k_out[b]) - float(k_in[b]) * s)
        print(f"d {d} {layout} {form} utt {b} g {bt.utts[b][1]} p {bt.p[b]} w {bt.w[b]} phi {bt.phi[b]}: s {s:.9f} scale {float(scale[b]):.9f} "
              f"|ds| {err_s:.3e} <= {bs:.3e}  |dcoef| {err_c:.3e} <= {abs(float(k_in[b])) * bc:.3e}")
        assert err_s <= bs, (b, err_s, bs)
        assert err_c <= abs(float(k_in[b])) * bc, (b, err_c, bc)
        if bt.active(b):
            assert torch.equal(k_out[b], k_in[b] * scale[b])               # the one fp32 multiply
        else:                                                              # phi == 0 or unguided: a bit copy, scale exactly 1
            assert float(scale[b]) == 1.0 and _bits(k_out)[b] == _bits(k_in)[b]
    if form == "struct":                                                   # every other word of the struct is copied
        keep = [0, 1, 3, 4, 5, 6, 7]
        assert torch.equal(_bits(out)[:, keep], _bits(cin)[:, keep])
    # NaN in every row that is not read changes nothing, and a second run gives the same bits
    scale_n, out_n, _ = run(bt, form, nan=True)
    assert torch.isfinite(scale_n).all() and torch.isfinite(out_n[:, :6] if form == "struct" else out_n).all()
    assert torch.equal(_bits(scale_n), _bits(scale)) and torch.equal(_bits(out_n), _bits(out))
    scale_2, out_2, _ = run(bt, form)
    assert torch.equal(_bits(scale_2), _bits(scale)) and torch.equal(_bits(out_2), _bits(out))


@pytest.mark.parametrize("layout", ["doubled", "mixed"])
def test_all_zero_eps_gives_one(cases, layout):
    bt, _ = cases(256, layout)
    scale, out, cin = run(bt, zero=True)
    assert (scale == 1.0).all() and torch.equal(_bits(out), _bits(cin))


@pytest.mark.parametrize("d", [64, 256, 768])
def test_an_utterance_has_the_same_bits_wherever_it_stands(cases, d):
    bt, _ = cases(d, "doubled")
    scale, _, _ = run(bt, nan=True)
    probes = [b for b in range(bt.B) if bt.active(b)]
    assert any(bt.utts[b][1] * d > 2 * CHUNK for b in probes)              # a several-chunk utterance is among them
    # the grid under-reported: one column strides over every utterance's chunks
    scale_1, _, _ = run(bt, nan=True, max_N=1)
    assert torch.equal(_bits(scale_1), _bits(scale))
    # every rescaled utterance again: first of a batch of two with another neighbour, doubled and mixed, exact and under-reported max_N
    for b in probes:
        other = (40 + b, 3, 1)
        for guided in (None, [True, False], [True, True]):
            two = Batch(d, [bt.utts[b], other], [bt.w[b], 3.0], [bt.phi[b], 0.9], guided)
            for max_N in (None, 2):
                s2, _, _ = run(two, nan=True, max_N=max_N)
                assert _bits(s2)[0] == _bits(scale)[b], (b, guided, max_N, float(s2[0]), float(scale[b]))
    # ... and last of a reversed batch
    rev = Batch(d, bt.utts[::-1], bt.w[::-1], bt.phi[::-1])
    s_rev, _, _ = run(rev, nan=True)
    assert torch.equal(_bits(s_rev.flip(0)), _bits(scale))


def test_out_of_range_tables_behave_as_their_clamped_values(cases):
    d = 256
    bt, _ = cases(d, "mixed")
    scale, out, _ = run(bt)
    B, G, S, S_G = bt.B, bt.G, bt.S, bt.S_G
    # prompt lengths: negative -> 0, beyond the utterance -> n_b - 1
    bad_p, good_p = list(bt.p), list(bt.p)
    bad_p[0], good_p[0] = -5, 0
    bad_p[4], good_p[4] = 10 ** 6, bt.n[4] - 1
    bad_p[7], good_p[7] = bt.n[7], bt.n[7] - 1
    a, b = run(bt, prompt=bad_p), run(bt, prompt=good_p)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert bt.active(4) and bt.w[4] == 5.0 and _bits(a[0])[4] != _bits(scale)[4]    # (the clamped value is another region: it was used)
    # no prompt lengths at all: P_b = 0
    a, b = run(bt, with_prompt=False), run(bt, prompt=[0] * B)
    assert torch.equal(_bits(a[0]), _bits(b[0]))
    # partners: below -1 -> -1 (unguided: a bit copy), beyond G - 1 -> G - 1
    bad_t, good_t = list(bt.partner), list(bt.partner)
    bad_t[0], good_t[0] = -9, -1
    last = max(range(B), key=lambda j: bt.partner[j])
    bad_t[last] = G + 50
    a, b = run(bt, partner=bad_t), run(bt, partner=good_t)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and float(a[0][0]) == 1.0
    # offsets: the first utterance's start below 0 -> 0 and (doubled layout, where that offset is nobody's start) the last one's end
    # beyond the S rows -> S: the table then says what the true one says
    bad_o = list(bt.offsets)
    bad_o[0] = -3
    a = run(bt, offsets=bad_o)
    assert torch.equal(_bits(a[0]), _bits(scale)) and torch.equal(_bits(a[1]), _bits(out))
    db, _ = cases(d, "doubled")
    bad_o = list(db.offsets)
    bad_o[0], bad_o[B] = -3, S + 1000
    a, b = run(db, offsets=bad_o), run(db)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    # a copy's start below S -> S, beyond the copies -> their last n_b rows
    bad_o, good_o = list(bt.offsets), list(bt.offsets)
    g0 = next(j for j in range(B) if bt.partner[j] == 0)
    gl = last
    bad_o[B + bt.partner[g0]], good_o[B + bt.partner[g0]] = 5, S            # below S -> S
    bad_o[B + bt.partner[gl]], good_o[B + bt.partner[gl]] = 2 ** 30, S + S_G - bt.n[gl]   # beyond -> the last n_b rows of the copies
    a, b = run(bt, offsets=bad_o), run(bt, offsets=good_o)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    # phi outside [0, 1] clamps on the device
    hi = Batch(d, bt.utts, bt.w, [1.75 if p == 1.0 else (-0.5 if p == 0.0 else p) for p in bt.phi], bt.guided)
    a = run(hi)
    assert torch.equal(_bits(a[0]), _bits(scale)) and torch.equal(_bits(a[1]), _bits(out))
