"""The elementwise bound of tests/attn_train_fwd_ref.py on the training attention forward, on the CPU: on every data set the GPU tests
use it passes a model of the kernel's arithmetic (bf16 q', fp32 scores, an octave maximum, bf16 probabilities, the row sum of their
roundings, fp32 accumulation, the residual add) on every element of O, lse, both streams and O beside the stream; it flags each bug the
kernel can have — an unmasked ragged key tail, a stale ring buffer, a dropout mask at the wrong index, head or row, a missing keep scale,
a masked row sum, lse in the wrong domain or slot, a dropped or misread residual, O beside the stream taken as a difference — and its lse
part stays at or below 2^-7 log2 units.  This is what makes test_gpu_attention_train_fwd_elementwise.py's passing mean something."""
import pytest
import torch

import attn_train_fwd_ref as R

CASES = R.all_cases()
FLAGGED = 2.0     # a mutation must leave a bound by this factor (test_attention_bound.py's)


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    cid, kw = request.param
    c = R.build(cid, kw)
    resid = R.make_resid(c)
    return cid, c, resid, R.reference(c, resid)


def _stored(got):
    return {n: t.to(torch.bfloat16).float() if R.BF16_STORED[n] else t for n, t in got.items()}


def test_bound_passes_the_kernels_arithmetic_on_every_element(case):
    cid, c, resid, ref = case
    r = R.ratios(_stored(R.emulate(c, resid)), ref)
    print("unmutated", cid, {n: round(x, 3) for n, x in r.items()})
    for n, x in r.items():
        assert x <= 1.0, f"the bound is too tight for the kernel's own rounding on {n}: {x:.3f}"


def test_lse_bound_stays_below_2_to_the_minus_7(case):
    cid, c, _, ref = case
    worst = float(ref.e_L.max())
    print("lse bound", cid, f"{worst:.3e}")
    assert worst <= 2.0 ** -7


def test_bound_flags_each_mutation(case):
    cid, c, resid, ref = case
    for m in R.mutations(c):
        r = R.ratios(_stored(R.emulate(c, resid, mutate=m)), ref)
        print(cid, m, {n: round(x, 2) for n, x in r.items() if x > 1.0})
        assert max(r.values()) > FLAGGED, f"mutation {m} not flagged: {r}"
    # recorded, not asserted: scores from c (q.k) on the raw q, the dk,dv kernel's definition, in units of this bound
    r = R.ratios(_stored(R.emulate(c, mutate="raw_q_scores")), ref)
    print(cid, "raw_q_scores (recorded)", {n: round(x, 3) for n, x in r.items()})


DENSE_CASES = [c for c in CASES if not c[0].startswith("packed")]     # (the older kernel has no packed form)


@pytest.mark.parametrize("cid,kw", DENSE_CASES, ids=[c[0] for c in DENSE_CASES])
def test_older_kernels_definition_passes_its_own_reference(cid, kw):
    """attn_flags 8192: scores c (q.k) on the raw q; the model of that arithmetic against reference(raw_q=True)"""
    c = R.build(cid, kw)
    resid = R.make_resid(c)
    r = R.ratios(_stored(R.emulate(c, resid, raw_q=True)), R.reference(c, resid, raw_q=True))
    print("raw q, unmutated", cid, {n: round(x, 3) for n, x in r.items()})
    assert max(r.values()) <= 1.0


def test_every_mutation_is_exercised_somewhere():
    seen = set()
    for cid, kw in CASES:
        seen.update(R.mutations(R.build(cid, kw)))
    assert seen == {"unmasked_tail", "stale_key_tile", "swapped_mask", "other_head_mask", "packed_global_mask", "no_keep_scale",
                    "masked_rowsum", "ln_not_log2", "lse_head_swap", "lse_wrong_slot", "resid_dropped", "resid_from_out",
                    "o_beside_is_delta"}
