"""-m gpu: the packed guided update (ditto_guided_update_packed, csrc/guided_packed.hip) held to a kernel that shares none of its span
code: the padded ditto_guided_update (csrc/guided.hip) on the same utterances padded to [B, N, d], which tests/test_gpu_guided_update.py
pins to the torch chain it replaced.  The tag, prompt and window tests take their expected values from the unprompted packed entry,
and all of them run one kernel; this is that kernel's own anchor.

Every valid row of both halves must be torch.equal — with a noise buffer, without noise and with Philox noise alike: the Philox quad
index is local to the utterance in both layouts.  d = 64 and utterances of 1, 5 and 130 rows: a single row, a partial workgroup (80
quads) and several workgroups in a grid column (2080 quads = 9 workgroups), N = 130.  Guard rows around every packed buffer catch a
write outside it."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8            # rows in front of and behind every packed buffer
D, LENS = 64, (1, 5, 130)
B, N, S = len(LENS), max(LENS), sum(LENS)
CU = [0, 1, 6, 136]
STEP = 49


def _guarded(t, fill):
    g = torch.full((GUARD, t.shape[1]), fill, dtype=t.dtype, device=DEV)
    pool = torch.cat([g, t, g]).contiguous()
    return pool, pool[GUARD:GUARD + t.shape[0]]


def _padded(packed):
    """[S, d] -> [B, N, d]; the padding rows hold NaN (the padded kernel reads nothing there)"""
    out = torch.full((B, N, D), float("nan"), device=DEV)
    for b, n in enumerate(LENS):
        out[b, :n] = packed[CU[b]:CU[b + 1]]
    return out


@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("noise", ["none", "buffer", "philox"])
def test_packed_update_equals_the_padded_update_on_every_valid_row(noise, cfg_on):
    lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
    halves = 2 if cfg_on else 1
    x = hash_normal((S, D), "anchor_x", 1).to(DEV)
    eps = hash_normal((halves * S, D), "anchor_eps", 2).to(DEV)
    z = hash_normal((S, D), "anchor_z", 3).to(DEV) if noise == "buffer" else None
    seeds = torch.tensor([5, -6, 2 ** 40 + 7], dtype=torch.int64, device=DEV) if noise == "philox" else None
    a, ce, cz, w = (torch.tensor(v, device=DEV) for v in ([0.9, 1.0, 1.1], [-0.2, -0.05, 0.1], [0.4, 0.5, 0.6], [2.0, 2.5, 3.0]))
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    coef = (ptr(w) if cfg_on else None, a.data_ptr(), ce.data_ptr(), cz.data_ptr())

    # expected: the padded entry on [B, N, d] ([2B, N, d] under CFG: the conditional utterances, then the unconditional ones)
    want = torch.cat([_padded(x)] * halves)
    eps_pad = torch.cat([_padded(eps[h * S:(h + 1) * S]) for h in range(halves)])
    z_pad = None if z is None else _padded(z)
    sl = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    hip.check(lib.ditto_guided_update(want.data_ptr(), eps_pad.data_ptr(), ptr(z_pad), ptr(seeds), STEP, *coef, sl.data_ptr(), B, N, D,
                                      int(cfg_on), st))

    x_pool, got = _guarded(torch.cat([x] * halves), 7.0)
    eps_pool, eps_g = _guarded(eps, float("nan"))
    z_pool, z_g = (None, None) if z is None else _guarded(z, float("nan"))
    eps_before = eps_pool.clone()
    cu = torch.tensor(CU, dtype=torch.int32, device=DEV)
    hip.check(lib.ditto_guided_update_packed(got.data_ptr(), eps_g.data_ptr(), ptr(z_g), ptr(seeds), STEP, *coef, cu.data_ptr(), B, S, N,
                                             D, int(cfg_on), st))
    for h in range(halves):
        for b, n in enumerate(LENS):
            rows = got[h * S + CU[b]:h * S + CU[b + 1]]
            assert torch.isfinite(rows).all() and torch.equal(rows, want[h * B + b, :n]), f"half {h}, utterance {b}"
    assert not torch.equal(got, torch.cat([x] * halves))
    assert torch.all(x_pool[:GUARD] == 7.0) and torch.all(x_pool[-GUARD:] == 7.0)
    assert torch.equal(eps_pool.view(torch.int32), eps_before.view(torch.int32)), "eps2 was written"
    if z_pool is not None:
        assert torch.isnan(z_pool[:GUARD]).all() and torch.isnan(z_pool[-GUARD:]).all()
