"""The elementwise bound of tests/attn_ref.py, on the CPU: it passes a model of the kernels' arithmetic (bf16 probabilities, fp32 or
bf16-rounded row sums), and it flags each of the bugs a fused attention kernel has had or could have — a stale score block, a
key tile missing from the numerator or the row sum, an unmasked partial tile, a residual added twice, not at all or from the
wrong row — on the data the GPU tests use.  This is what makes the GPU tests' passing mean something."""
import pytest
import torch

from attn_ref import bound, emulate, make_case, reference, worst_ratio
from gpu_util import asym

SHAPES = [(1, 2, 300, 1024), (1, 2, 300, 471), (2, 1, 256, 191)]


def _stored(x, bf):
    x = x.float()
    return x.to(torch.bfloat16).float() if bf else x


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "B%d_H%d_Sq%d_Skv%d" % s)
def case(request):
    B, H, Sq, Skv = request.param
    q, k, v, _ = make_case(B, H, Sq, Skv, seed=70)
    return (B, H, Sq, Skv), (q, k, v), reference(q, k, v, B, H, Sq, Skv, 64), asym((B * Sq, H * 64), 73)


@pytest.mark.parametrize("stream_bf16", [False, True], ids=["fp32_stream", "bf16_stream"])
def test_bound_passes_the_kernels_arithmetic_and_flags_each_mutation(case, stream_bf16):
    (B, H, Sq, Skv), (q, k, v), (o, wabs, s1), resid = case
    r = _stored(resid, stream_bf16)
    want, e = bound(o, wabs, s1, Skv, 64, resid=r)
    for rowsum_bf16 in (False, True):
        got = _stored(emulate(q, k, v, B, H, Sq, Skv, 64, rowsum_bf16=rowsum_bf16) + r, stream_bf16)
        ratio = worst_ratio(got, want, e, stream_bf16)
        assert ratio < 0.8, f"the bound is too tight for the kernels' own rounding (row sum bf16 = {rowsum_bf16}): {ratio:.3f}"
    nkt = (Skv + 63) // 64
    mutations = ["stale_block", "drop_num", "drop_sum"] + (["unmasked"] if Skv % 64 else [])
    for m in mutations:
        tile = max(1, min(nkt // 2, nkt - 2)) if m == "stale_block" else nkt // 2   # stale_block: a whole tile after tile 0
        got = _stored(emulate(q, k, v, B, H, Sq, Skv, 64, mutate=m, tile=tile) + r, stream_bf16)
        assert worst_ratio(got, want, e, stream_bf16) > 2.0, f"mutation {m} not flagged"
    neighbour = r.view(B, Sq, -1).roll(1, dims=1).reshape(B * Sq, -1)
    for name, got in (("residual twice", o + 2 * r), ("no residual", o), ("neighbouring row's residual", o + neighbour)):
        assert worst_ratio(_stored(got, stream_bf16), want, e, stream_bf16) > 2.0, f"{name} not flagged"


def test_bound_flags_a_kernel_that_drops_one_key():
    """Sharper still: one key missing (the boundary of a partial tile off by one) on a row it dominates."""
    B, H, Sq, Skv = 1, 1, 64, 127
    q, k, v, _ = make_case(B, H, Sq, Skv, seed=80)
    o, wabs, s1 = reference(q, k, v, B, H, Sq, Skv, 64)
    want, e = bound(o, wabs, s1, Skv, 64)
    o2, _, _ = reference(q, k[:Skv - 1], v[:Skv - 1], B, H, Sq, Skv - 1, 64)
    assert worst_ratio(_stored(o2, True), want, e, True) > 2.0
