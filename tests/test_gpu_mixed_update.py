"""-m gpu: the update of a step in which only some utterances are guided (csrc/guided_mixed.hip, ditto_guided_update_packed_mixed).

Expected values come from the EXISTING per-utterance-tag entry with prompts, ditto_guided_update_packed_tags_prompt: its cfg = 1 form
run on the guided utterances compacted into a pair batch [x_G; x_G] gives their generated rows in both copies, its cfg = 0 form on the
whole batch gives the unguided ones; everything is torch.equal.  Prompt rows of x2 hold a sentinel that must survive, those of eps2
and of the noise buffer hold NaN (they are not read); NaN guard rows around every buffer must stay bit for bit as they were, and a
read from them would show as NaN in the result."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
D = 256
N = [1, 33, 64, 95]
P = [0, 5, 0, 94]
PARTNER = [-1, 0, -1, 1]
B, S = len(N), sum(N)
NOISES = ["philox", "none", "buffer"]


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


CU = _cu(N)


@pytest.fixture(scope="module")
def data():
    """the inputs every test shares (read-only): the state, eps for the B utterances and for B copies, a noise buffer, coefficients"""
    k = torch.arange(B, dtype=torch.float32)
    tags_l = [49, 17, 0xFFFFFFF0, 3]
    return dict(x=hash_normal((S, D), "mx_x", 1).to(DEV), eps_c=hash_normal((S, D), "mx_eps", 2).to(DEV),
                eps_u=hash_normal((S, D), "mx_eps", 3).to(DEV), z=hash_normal((S, D), "mx_z", 4).to(DEV),
                a=(0.9 + 0.1 * k).to(DEV), ce=(-0.2 + 0.15 * k).to(DEV),
                cz=torch.tensor([0.0, 0.4, 0.3, 0.0], device=DEV),        # a sigma = 0 utterance in each class: no draw there
                w=(2.0 + 0.5 * k).to(DEV), seeds=torch.tensor([5, -6, 2 ** 40 + 7, 8], dtype=torch.int64, device=DEV),
                tags=_i32([t - (1 << 32) if t >= 1 << 31 else t for t in tags_l]))


def _rows(b, lo=0):
    return torch.arange(CU[b] + lo, CU[b + 1], device=DEV)


def _guarded(t):
    g = torch.full((GUARD, t.shape[1]), float("nan"), dtype=t.dtype, device=DEV)
    pool = torch.cat([g, t, g]).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _existing(dt, noise, idx, prompts, cfg_on):
    """ditto_guided_update_packed_tags_prompt over the utterances `idx` compacted into a batch of their own ([x; x] under cfg, eps_u
    behind eps_c): (the result, the rows of utterance k's generated part in one half, rows of one half)"""
    rows = torch.cat([_rows(b) for b in idx])
    lens = [N[b] for b in idx]
    Sk = sum(lens)
    sel = torch.tensor(idx, device=DEV)
    x = torch.cat([dt["x"][rows]] * (2 if cfg_on else 1)).contiguous()
    eps = torch.cat([dt["eps_c"][rows]] + ([dt["eps_u"][rows]] if cfg_on else [])).contiguous()
    z = dt["z"][rows].contiguous() if noise == "buffer" else None
    seeds = dt["seeds"][sel].contiguous() if noise == "philox" else None
    cu = _cu(lens)
    keep = {k: dt[k][sel].contiguous() for k in ("tags", "w", "a", "ce", "cz")}      # (alive until the call has been queued)
    cud, pld = _i32(cu), _i32([prompts[b] for b in idx])
    hip.check(hip.lib().ditto_guided_update_packed_tags_prompt(
        x.data_ptr(), eps.data_ptr(), _ptr(z), _ptr(seeds), keep["tags"].data_ptr(), keep["w"].data_ptr() if cfg_on else None,
        keep["a"].data_ptr(), keep["ce"].data_ptr(), keep["cz"].data_ptr(), cud.data_ptr(), pld.data_ptr(), len(idx), Sk, max(lens), D,
        int(cfg_on), _s()))
    torch.cuda.synchronize()
    gen = [torch.arange(cu[k] + prompts[b], cu[k + 1], device=DEV) for k, b in enumerate(idx)]
    return x, gen, Sk


class Mixed:
    """one call of the new entry: x2 / eps2 [S + S_G, d] with sentinel / NaN prompt rows, inside NaN guards"""

    def __init__(self, dt, noise, partner, prompts, G=None):
        self.guided = [b for b in range(B) if partner[b] >= 0] if G is None else G
        g = self.guided
        self.cu_g = _cu([N[b] for b in g])
        self.S_G = self.cu_g[-1]
        x = torch.cat([dt["x"]] + [dt["x"][_rows(b)] for b in g])
        eps = torch.cat([dt["eps_c"]] + [dt["eps_u"][_rows(b)] for b in g])
        z = dt["z"].clone() if noise == "buffer" else None
        self.prompt_rows = []
        for b in range(B):
            if prompts is None or prompts[b] == 0:
                continue
            at = [CU[b]] + ([S + self.cu_g[g.index(b)]] if b in g else [])
            for lo in at:
                r = torch.arange(lo, lo + prompts[b], device=DEV)
                self.prompt_rows.append(r)
                x[r] = (torch.arange(len(r) * D, dtype=torch.float32, device=DEV).reshape(-1, D) % 97) + 1000.0
                eps[r] = float("nan")
            if z is not None:
                z[CU[b]:CU[b] + prompts[b]] = float("nan")
        self.x_pool, self.x = _guarded(x)
        self.eps_pool, self.eps = _guarded(eps)
        self.z_pool, self.z = _guarded(z) if z is not None else (None, None)
        self.x_before = self.x_pool.clone()
        offsets, part = _i32(CU + [S + c for c in self.cu_g[1:]]), _i32(partner)
        pld = None if prompts is None else _i32(prompts)
        hip.check(hip.lib().ditto_guided_update_packed_mixed(
            self.x.data_ptr(), self.eps.data_ptr(), _ptr(self.z), _ptr(dt["seeds"]) if noise == "philox" else None,
            dt["tags"].data_ptr(), dt["w"].data_ptr(), dt["a"].data_ptr(), dt["ce"].data_ptr(), dt["cz"].data_ptr(),
            offsets.data_ptr(), part.data_ptr(), _ptr(pld), B, len(g), S, self.S_G, max(N), D, _s()))
        torch.cuda.synchronize()

    def copy_rows(self, b, lo=0):
        k = self.guided.index(b)
        return torch.arange(S + self.cu_g[k] + lo, S + self.cu_g[k + 1], device=DEV)

    def check_guards(self):
        assert _same_bits(self.x_pool[:GUARD], self.x_before[:GUARD]) and _same_bits(self.x_pool[-GUARD:], self.x_before[-GUARD:])
        assert torch.isnan(self.x_pool[:GUARD]).all() and torch.isnan(self.x_pool[-GUARD:]).all()

    def check_untouched(self):
        for r in self.prompt_rows:
            assert _same_bits(self.x[r], self.x_before[GUARD:][r]), "a prompt row of x2 was written"
        self.check_guards()


@pytest.mark.parametrize("noise", NOISES)
def test_mixed_step_is_the_cfg_kernel_on_the_guided_pair_and_the_plain_kernel_on_the_rest(data, noise):
    m = Mixed(data, noise, PARTNER, P)
    guided, rest = [1, 3], [0, 2]
    want, gen, Sk = _existing(data, noise, guided, P, True)
    assert torch.isfinite(want).all()
    for k, b in enumerate(guided):
        assert torch.equal(m.x[_rows(b, P[b])], want[gen[k]]), f"utterance {b}, conditional rows"
        assert torch.equal(m.x[m.copy_rows(b, P[b])], want[gen[k] + Sk]), f"utterance {b}, unconditional copy"
    plain, gen, _ = _existing(data, noise, list(range(B)), P, False)
    for b in rest:
        assert torch.isfinite(m.x[_rows(b, P[b])]).all()
        assert torch.equal(m.x[_rows(b, P[b])], plain[gen[b]]), f"utterance {b}, unguided"
    assert not torch.equal(m.x[_rows(1, P[1])], plain[gen[1]])          # the guidance matters
    m.check_untouched()


@pytest.mark.parametrize("prompts", [P, None], ids=["prompts", "no_prompts"])
@pytest.mark.parametrize("noise", NOISES)
def test_identity_partner_is_the_cfg_kernel_and_no_partner_is_the_plain_kernel(data, noise, prompts):
    pl = prompts or [0] * B
    m = Mixed(data, noise, list(range(B)), prompts)
    want, gen, _ = _existing(data, noise, list(range(B)), pl, True)
    for b in range(B):
        assert torch.equal(m.x[_rows(b, pl[b])], want[gen[b]]) and torch.equal(m.x[m.copy_rows(b, pl[b])], want[gen[b] + S])
    m.check_untouched()
    m = Mixed(data, noise, [-1] * B, prompts)
    assert m.S_G == 0 and m.x.shape[0] == S
    want, gen, _ = _existing(data, noise, list(range(B)), pl, False)
    for b in range(B):
        assert torch.equal(m.x[_rows(b, pl[b])], want[gen[b]])
    assert torch.isfinite(m.x[torch.cat(gen)]).all()
    m.check_untouched()


@pytest.mark.parametrize("noise", NOISES)
def test_out_of_range_partners_touch_nothing_outside_the_buffers(data, noise):
    """the device clamps partner[b] into [-1, G - 1]: wrong rows, never an access outside the S + S_G rows — the NaN guards keep
    their bits, and nothing read from them reaches a row"""
    m = Mixed(data, noise, [5, -7, 1, 2 ** 31 - 1], None, G=[1, 3])
    m.check_guards()
    assert torch.isfinite(m.x).all()                                   # eps2 and the noise have NaN only in their guards
    before = m.x_before[GUARD:GUARD + S + m.S_G]
    assert not torch.equal(m.x[_rows(1)], before[_rows(1)])            # -7 -> no partner: the utterance is still updated ...
    assert _same_bits(m.x[m.copy_rows(1)], before[m.copy_rows(1)])     # ... and copy 0, which no clamped partner names, is not


@pytest.mark.parametrize("noise", NOISES)
def test_a_copy_shorter_than_its_utterance_is_moved_inside_the_buffers(data, noise):
    """the copies in the order [3, 1]: the last copy has 33 rows.  Utterances 2 (64 rows) and 3 (95 rows) name it: the copy's span
    keeps the utterance's own length and its first row is clamped into [S, S + S_G - n_b], so nothing is read or written behind row
    S + S_G (NaN guards there, in x2, eps2 and the noise alike) and the utterances' own rows are updated in full, with guidance"""
    m = Mixed(data, noise, [-1, 0, 1, 1], None, G=[3, 1])
    assert m.S_G == 128 and m.cu_g == [0, 95, 128]
    m.check_guards()
    assert torch.isfinite(m.x).all()
    plain, gen, _ = _existing(data, noise, list(range(B)), [0] * B, False)
    for b in (2, 3):
        assert not torch.equal(m.x[_rows(b)], plain[gen[b]])             # guided: eps_u came from rows inside the buffer
    assert torch.equal(m.x[_rows(0)], plain[gen[0]])


@pytest.mark.parametrize("noise", NOISES)
def test_an_utterance_longer_than_all_the_copies_is_updated_without_guidance(data, noise):
    """one copy of one row (utterance 0's), named by everyone: utterances 1, 2, 3 are longer than S_G = 1, get no copy and the
    non-CFG arithmetic over all their rows; utterance 0 is guided"""
    m = Mixed(data, noise, [0, 0, 0, 0], None, G=[0])
    assert m.S_G == 1
    m.check_guards()
    plain, gen, _ = _existing(data, noise, list(range(B)), [0] * B, False)
    for b in (1, 2, 3):
        assert torch.equal(m.x[_rows(b)], plain[gen[b]])
    want, gen, Sk = _existing(data, noise, [0], [0] * B, True)
    assert torch.equal(m.x[_rows(0)], want[gen[0]]) and torch.equal(m.x[m.copy_rows(0)], want[gen[0] + Sk])
