"""The elementwise bound of tests/attn_ref.py on the GEMM-composed attention (any head_dim but 64), on the CPU: with the reference
restricted to each row's visible keys it passes a model of that path's arithmetic (fp32 scores, normalised probabilities rounded
to bf16, fp32 P V), and on the data of make_masked_case it flags each of the bugs a mask or a chunk of (batch, head) pairs can
have: one visible key too few, one too many, the padded batch's causal offset taken for the utterance's own, another head's V.
This is what makes tests/test_gpu_attention_composed_elementwise.py's passing mean something."""
import pytest
import torch

from attn_ref import LOG2E, bound, emulate_composed, make_masked_case, reference, visible_keys, worst_ratio

# B, H, Sq, Skv, dh, causal, q_len, kv_len
CASES = [
    (1, 1, 40, 40, 1536, True, None, None),                  # the dense causal entry
    (1, 1, 70, 33, 128, True, None, None),                   # Sq > Skv: the first 37 rows see nothing
    (2, 2, 33, 70, 128, True, [33, 5], [70, 64]),            # kl - ql = 37, 59 against Skv - Sq = 37
    (2, 1, 70, 70, 768, True, [1, 65], [1, 64]),             # length 1; kl < ql: row 0 of utterance 1 sees nothing
    (3, 2, 33, 70, 128, False, [33, 5, 20], [70, 1, 33]),
    (2, 1, 66, 130, 768, False, None, [64, 65]),
    (2, 2, 64, 66, 1536, False, [64, 1], [65, 66]),
]


def _id(c):
    return "B%d_H%d_%dx%d_dh%d_%s" % (*c[:5], "causal" if c[5] else "full") + ("" if c[6] is None and c[7] is None else "_len")


def _stored(x, bf):
    x = x.float()
    return x.to(torch.bfloat16).float() if bf else x


@pytest.fixture(scope="module", params=CASES, ids=_id)
def case(request):
    B, H, Sq, Skv, dh, causal, q_len, kv_len = request.param
    q, k, v, scale = make_masked_case(B, H, Sq, Skv, dh, 300, q_len, kv_len, causal)
    vis = visible_keys(B, Sq, Skv, q_len, kv_len, causal)
    o, wabs, s1 = reference(q, k, v, B, H, Sq, Skv, dh, scale * LOG2E, vis=vis)
    return request.param, (q, k, v, scale), vis, bound(o, wabs, s1, Skv, dh)


def _applicable(m, B, H, Sq, Skv, causal, q_len, kv_len, vis):
    """can this shape show the mutation at all?  (decided on the masks, never on a ratio)"""
    if m == "wrong_head":
        return H > 1
    if m == "one_more":        # some valid row must have a further key in the buffer
        valid = visible_keys(B, Sq, Skv, q_len, None, False) > 0                   # rows below q_len
        return bool(((vis < Skv) & valid).any())
    if m == "padded_offset":   # the two offsets must give some row another count
        return causal and not torch.equal(visible_keys(B, Sq, Skv, q_len, kv_len, True, padded_offset=True), vis)
    return True


@pytest.mark.parametrize("out_bf16", [True, False], ids=["bf16_out", "fp32_out"])
def test_bound_passes_the_composed_arithmetic_and_flags_each_mutation(case, out_bf16):
    (B, H, Sq, Skv, dh, causal, q_len, kv_len), (q, k, v, scale), vis, (want, e) = case
    args = (q, k, v, B, H, Sq, Skv, dh, scale, q_len, kv_len, causal)
    got = _stored(emulate_composed(*args), out_bf16)
    ratio = worst_ratio(got, want, e, out_bf16)
    assert ratio < 0.8, f"the bound is too tight for the path's own rounding: {ratio:.3f}"
    assert bool((got[(vis == 0).reshape(-1)] == 0).all()), "a row that sees no key is not exactly 0"
    flagged = 0
    for m in ("one_fewer", "one_more", "padded_offset", "wrong_head"):
        if not _applicable(m, B, H, Sq, Skv, causal, q_len, kv_len, vis):
            continue
        r = worst_ratio(_stored(emulate_composed(*args, mutate=m), out_bf16), want, e, out_bf16)
        assert r > 2.0, f"mutation {m} not flagged: {r:.3f}"
        flagged += 1
    assert flagged >= 1


def test_every_mutation_is_applicable_somewhere():
    seen = set()
    for B, H, Sq, Skv, dh, causal, q_len, kv_len in CASES:
        vis = visible_keys(B, Sq, Skv, q_len, kv_len, causal)
        seen |= {m for m in ("one_fewer", "one_more", "padded_offset", "wrong_head")
                 if _applicable(m, B, H, Sq, Skv, causal, q_len, kv_len, vis)}
    assert seen == {"one_fewer", "one_more", "padded_offset", "wrong_head"}
    assert {c[4] for c in CASES} >= {128, 768, 1536}


def test_visible_keys_rule():
    """the helper against the rule written out, at the lengths of the issue's table"""
    vis = visible_keys(2, 33, 70, [33, 5], [70, 64], True)
    assert vis[0].tolist() == [i + 38 for i in range(33)]                       # off = 37: the last row sees all 70
    assert vis[1].tolist() == [i + 60 for i in range(5)] + [0] * 28             # off = 59
    assert visible_keys(1, 70, 33, None, None, True)[0].tolist() == [0] * 37 + list(range(1, 34))
    assert visible_keys(2, 4, 9, None, [1, 9], False).tolist() == [[1] * 4, [9] * 4]
    assert visible_keys(1, 4, 9, [0], [100], False).tolist() == [[9, 0, 0, 0]]    # lengths clamp to [1, full]


def test_reference_without_counts_is_unchanged():
    """vis = None is the old code path; a full count gives the same numbers"""
    q, k, v, scale = make_masked_case(2, 2, 9, 17, 128, 5)
    a = reference(q, k, v, 2, 2, 9, 17, 128, scale * LOG2E)
    b = reference(q, k, v, 2, 2, 9, 17, 128, scale * LOG2E, vis=visible_keys(2, 9, 17))
    for x, y in zip(a, b):
        assert torch.allclose(x, y, rtol=1e-12, atol=1e-300)
