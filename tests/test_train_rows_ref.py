"""train_rows_ref.py checked without a GPU: every reference against torch autograd in fp64, an fp32 emulation of every kernel's written
expression inside its bound on every case of the tables (`-s` prints EMU_RATIO lines: the worst ratio, < 1), a table of modelled defects
every one of which leaves its bound on these very inputs (DEFECT_RATIO lines: the least ratio, > 1 by a wide margin), and the library's
size helpers (host code) against their restatement."""
import math

import pytest
import torch

import train_rows_ref as T
from ditto_tts_amd import hip
from gemm_epi_ref import worst_ratio

D = torch.float64


def emu(what, r):
    print(f"EMU_RATIO {what} {r:.3f}")
    assert r < 1.0, (what, r)


def defect(what, r, least=10.0):
    print(f"DEFECT_RATIO {what} {r:.3g}")
    assert r > least, (what, r)


def stored(v32):
    """what a kernel stores as bf16, as fp64"""
    return T.bf(v32).double()


# ------------------------------------------------------------------ autograd ------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [True, False])
def test_ln_reference_is_autograd(gamma):
    c = T.ln_case(7, 64, 3)
    x = c["x"].double().requires_grad_()
    g = c["gamma"].double().requires_grad_()
    b = torch.zeros(64, dtype=D, requires_grad=True)
    y = torch.nn.functional.layer_norm(x, (64,), g if gamma else None, b if gamma else None, 1e-5)
    y.backward(c["dy"].double())
    r = T.ln_bwd_ref(c["x"], c["dy"], c["gamma"] if gamma else None, c["acc0"])
    assert torch.allclose(r["acc"] - c["acc0"].double(), x.grad, rtol=1e-11, atol=1e-13)
    if gamma:
        assert torch.allclose(r["dgamma"][0], g.grad, rtol=1e-11, atol=1e-13) and torch.allclose(r["dbeta"][0], b.grad, rtol=1e-12)


def test_adaln_reference_is_autograd_per_utterance():
    c = T.adaln_case([4, 1, 6], 64, 5)
    S = c["cu"][-1]
    utt = torch.repeat_interleave(torch.arange(3), torch.tensor([4, 1, 6]))
    sc = torch.zeros(3, 64, dtype=D, requires_grad=True)
    sh = torch.zeros(3, 64, dtype=D, requires_grad=True)
    xh = torch.nn.functional.layer_norm(c["x"].double(), (64,), None, None, 1e-5)
    (xh * (1 + sc[utt]) + sh[utt]).backward(c["dy"].double())
    want, _ = T.adaln_packed_ref(c)
    assert S == 11 and torch.allclose(want, torch.cat([sc.grad, sh.grad], 1), rtol=1e-11, atol=1e-13)


def test_gated_reference_is_autograd():
    c = T.gated_case(5, 48, 7)
    a, g = c["a"].double().requires_grad_(), c["g"].double().requires_grad_()
    (torch.nn.functional.gelu(a) * torch.sigmoid(g)).backward(c["dy"].double())
    want, _, fl = T.gated_ref(c)
    assert torch.allclose(want, T.interleave(a.grad, g.grad), rtol=1e-10, atol=1e-300)
    assert 1e-8 < fl["cdf"] < 3e-6                                      # the rational form: a few 1e-7, as common.h says


def test_softmax_reference_is_autograd():
    c = T.softmax_case(3, 65, 9)
    keep = T.softmax_mask(c, 0.1)
    S = c["S"][:, :65].double().requires_grad_()
    ks = 1.0 / (1.0 - float(torch.tensor(0.1, dtype=torch.float32)))
    P = torch.softmax(S * T.SOFTMAX_SCALE, 1) * keep * ks
    P.backward(c["dP"][:, :65].double())
    r = T.softmax_rows_ref(c, 0.1)
    assert torch.allclose(r["P"][:, :65], P.detach(), rtol=1e-6, atol=0) and torch.allclose(r["dS"][:, :65], S.grad, rtol=1e-6, atol=1e-12)
    assert 0.02 < 1 - float(keep.mean()) < 0.25 and not r["P"][:, 65:].any()


@pytest.mark.parametrize("silu", [True, False])
def test_small_linear_reference_is_autograd(silu):
    c = T.small_linear_case(3, 65, 5, 11)
    x, W, b = (c[k].double().requires_grad_() for k in ("x", "W", "bias"))
    y = torch.nn.functional.linear(torch.nn.functional.silu(x) if silu else x, W, b)
    y.backward(c["dy"].double())
    assert torch.allclose(T.small_linear_ref(c, 0, silu)[0], y.detach(), rtol=1e-12)
    dW, _, db, _ = T.small_linear_ref(c, 1, silu)
    assert torch.allclose(dW, W.grad, rtol=1e-11, atol=1e-14) and torch.allclose(db, b.grad, rtol=1e-12)
    assert torch.allclose(T.small_linear_ref(c, 2, silu)[0], x.grad, rtol=1e-11, atol=1e-14)


# ------------------------------------------------------------ emulation inside, defects outside ------------------------------------------------------------
def test_ln_emulation_inside_and_defects_outside():
    worst = dict(acc=0.0, dgamma=0.0, dbeta=0.0)
    least = dict(neighbour_mean=math.inf, neighbour_rstd=math.inf, no_mean_g=math.inf)
    for (rows, d) in T.LN_STREAM_SHAPES:
        for form in T.LN_FORMS:
            c = T.ln_case(rows, d, 17 + rows + d, form)
            for gamma in (c["gamma"], None):
                r = T.ln_bwd_ref(c["x"], c["dy"], gamma, c["acc0"])
                acc, dg, db = T.ln_bwd_emulate(c["x"], c["dy"], gamma, c["acc0"])
                worst["acc"] = max(worst["acc"], worst_ratio(acc, r["acc"], r["e_acc"]))
                worst["dgamma"] = max(worst["dgamma"], worst_ratio(dg, r["dgamma"][0], r["e_dgamma"][0]))
                worst["dbeta"] = max(worst["dbeta"], worst_ratio(db, r["dbeta"][0], r["e_dbeta"][0]))
                if rows > 1:
                    for m in least:
                        bad, bdg, _ = T.ln_bwd_emulate(c["x"], c["dy"], gamma, c["acc0"], m)
                        least[m] = min(least[m], max(worst_ratio(bad, r["acc"], r["e_acc"]), worst_ratio(bdg, r["dgamma"][0], r["e_dgamma"][0])))
    for (rpg, groups, d) in T.LN_GROUP_SHAPES:                          # the group form: every group's sums over its own rows
        c = T.ln_case(rpg * groups, d, 23 + rpg + d)
        segs = [(g * rpg, (g + 1) * rpg) for g in range(groups)]
        r = T.ln_bwd_ref(c["x"], c["dy"], c["gamma"], c["acc0"], segs)
        for g, (lo, hi) in enumerate(segs):
            acc, dg, db = T.ln_bwd_emulate(c["x"][lo:hi], c["dy"][lo:hi], c["gamma"], c["acc0"][lo:hi])
            worst["acc"] = max(worst["acc"], worst_ratio(acc, r["acc"][lo:hi], r["e_acc"][lo:hi]))
            worst["dgamma"] = max(worst["dgamma"], worst_ratio(dg, r["dgamma"][g], r["e_dgamma"][g]))
            worst["dbeta"] = max(worst["dbeta"], worst_ratio(db, r["dbeta"][g], r["e_dbeta"][g]))
    for k, v in worst.items():
        emu("ln_" + k, v)
    for k, v in least.items():
        defect("ln_" + k, v, 100.0)


def test_ln_sums_defects_ragged_chunk_and_neighbour_group():
    """the last ragged chunk dropped from a column sum; an utterance's partial taken from its neighbour"""
    for rows, d in ((37, 64), (1100, 64)):
        c = T.ln_case(rows, d, 29 + rows)
        r = T.ln_bwd_ref(c["x"], c["dy"], None, c["acc0"])
        chunks = T.ln_chunks(rows, 1)
        rpc = (rows + chunks - 1) // chunks
        cut = (rows - 1) // rpc * rpc
        db = c["dy"][:cut].sum(0)
        defect(f"ln_dbeta_last_chunk_dropped_{rows}", worst_ratio(db, r["dbeta"][0], r["e_dbeta"][0]), 100.0)
        s, es = T.colsum_ref(r["acc"])
        defect(f"ln_colsum_last_chunk_dropped_{rows}", worst_ratio(r["acc"][:cut].float().sum(0), s, es), 100.0)
    c = T.adaln_case([40, 1, 17], 64, 31)
    want, e = T.adaln_packed_ref(c)
    defect("adaln_neighbour_utterance", worst_ratio(want.roll(1, 0).float(), want, e), 100.0)
    got = T.ln_bwd_ref(c["x"], c["dy"], None, None, [(0, 41)])["dgamma"]      # utterance 0's partial runs one row into utterance 1
    defect("adaln_partial_straddles", worst_ratio(got[0].float(), want[0, :64], e[0, :64]), 100.0)


def test_adaln_emulation_inside():
    w = 0.0
    for lens in T.ADALN_LENS:
        for d in T.ADALN_D:
            c = T.adaln_case(lens, d, 41 + d + lens[0])
            want, e = T.adaln_packed_ref(c)
            for b, (lo, hi) in enumerate(zip(c["cu"][:-1], c["cu"][1:])):
                _, dg, db = T.ln_bwd_emulate(c["x"][lo:hi], c["dy"][lo:hi], None, None)
                w = max(w, worst_ratio(torch.cat([dg, db]), want[b], e[b]))
    emu("adaln_dmod", w)


def test_gated_emulation_inside_and_defects_outside():
    w = dict(da=0.0, dg=0.0)
    least = dict(no_a_pdf=math.inf, sigmoid_sign=math.inf, unrounded_bias_sum=math.inf)
    for F in T.GATED_F:
        for M in T.GATED_M:
            c = T.gated_case(M, F, 51 + M + F)
            want, e, _ = T.gated_ref(c)
            da, dg = T.gated_emulate(c)
            got = T.interleave(stored(da), stored(dg))
            r = ((got - want).abs() - torch.ldexp(torch.ones_like(got), torch.frexp(got)[1] - 9)).clamp_min(0) / e
            rr = r.view(M, F // 16, 2, 16)
            w["da"], w["dg"] = max(w["da"], float(rr[:, :, 0].max())), max(w["dg"], float(rr[:, :, 1].max()))
            for m in ("no_a_pdf", "sigmoid_sign"):
                bda, bdg = T.gated_emulate(c, m)
                least[m] = min(least[m], worst_ratio(T.interleave(stored(bda), stored(bdg)), want, e, stored_bf16=True))
            if M > 1:
                s, es = T.colsum_ref(got)                                # the sums of what was stored ...
                bad = T.interleave(da, dg).double().sum(0).float()       # ... against the sums of the unrounded values
                least["unrounded_bias_sum"] = min(least["unrounded_bias_sum"], worst_ratio(bad, s, es))
    emu("gated_da", w["da"])
    emu("gated_dg", w["dg"])
    for k, v in least.items():
        defect("gated_" + k, v)


def test_softmax_emulation_inside_and_defects_outside():
    w = dict(P=0.0, dS=0.0)
    least = dict(mask_of_pair_bh=math.inf, mask_not_on_dP=math.inf, padding_not_zeroed=math.inf)
    for rpb in T.SOFTMAX_RPB:
        for Skv in T.SOFTMAX_SKV:
            c = T.softmax_case(rpb, Skv, 61 + Skv + rpb)
            for p in T.SOFTMAX_P:
                r = T.softmax_rows_ref(c, p)
                P, dS = T.softmax_emulate(c, p, r["keep"])
                w["P"] = max(w["P"], worst_ratio(stored(P), r["P"][:, :Skv], r["e_P"][:, :Skv], stored_bf16=True))
                w["dS"] = max(w["dS"], worst_ratio(stored(dS), r["dS"][:, :Skv], r["e_dS"][:, :Skv], stored_bf16=True))
                if p and Skv >= 63:
                    wrong = T.softmax_mask(c, p, bh0=0)                  # the streams of pairs 0 .. instead of bh0 ..
                    assert not torch.equal(wrong, r["keep"])
                    bP, bdS = T.softmax_emulate(c, p, wrong)
                    least["mask_of_pair_bh"] = min(least["mask_of_pair_bh"],
                                                   worst_ratio(stored(bP), r["P"][:, :Skv], r["e_P"][:, :Skv], stored_bf16=True),
                                                   worst_ratio(stored(bdS), r["dS"][:, :Skv], r["e_dS"][:, :Skv], stored_bf16=True))
                    _, bdS = T.softmax_emulate(c, p, r["keep"], torch.ones_like(r["keep"]))
                    least["mask_not_on_dP"] = min(least["mask_not_on_dP"],
                                                  worst_ratio(stored(bdS), r["dS"][:, :Skv], r["e_dS"][:, :Skv], stored_bf16=True))
                if c["ld"] > Skv:
                    pad = torch.full((c["nrows"], c["ld"] - Skv), 1e-3, dtype=D)    # whatever stood there
                    least["padding_not_zeroed"] = min(least["padding_not_zeroed"], worst_ratio(pad, r["P"][:, Skv:], r["e_P"][:, Skv:]))
    emu("softmax_P", w["P"])
    emu("softmax_dS", w["dS"])
    for k, v in least.items():
        defect("softmax_" + k, v, 100.0)


def test_small_linear_and_colsum_emulation_inside():
    w = 0.0
    for (B, I, O) in T.SMALL_LINEAR_CASES:
        c = T.small_linear_case(B, I, O, 71 + I)
        for silu in (True, False):
            y, e = T.small_linear_ref(c, 0, silu)
            w = max(w, worst_ratio(T.small_linear_emulate(c, 0, silu), y, e))
            dW, e, db, edb = T.small_linear_ref(c, 1, silu)
            gW, gb = T.small_linear_emulate(c, 1, silu)
            w = max(w, worst_ratio(gW, dW, e), worst_ratio(gb, db, edb))
            dx, e = T.small_linear_ref(c, 2, silu)
            w = max(w, worst_ratio(T.small_linear_emulate(c, 2, silu), dx, e))
    emu("small_linear", w)
    w = 0.0
    for (M, n, ld) in T.COLSUM_CASES:
        x = T.scaled_rows(M, ld, 81 + M)
        s, e = T.colsum_ref(x[:, :n].double())
        w = max(w, worst_ratio(x[:, :n].sum(0), s, e))
        if M >= 33:                                                      # the last ragged chunk dropped
            chunks = T.colsum_chunks(M, n)
            rpc = (M + chunks - 1) // chunks
            cut = (M - 1) // rpc * rpc                                   # the first row of the last chunk that has rows
            defect(f"colsum_last_chunk_dropped_{M}", worst_ratio(x[:cut, :n].sum(0), s, e), 5.0)   # 36 rows of 9000 under a 9001 u bound: 9
    emu("colsum", w)


def test_exact_references_and_their_defects():
    for (rows, cols, blk, mult, off) in T.PACK_CASES:
        m = T.pack_map(rows, blk, mult, off)
        assert len(set(m.tolist())) == rows and int(m[-1]) == int(m.max()) < T.pack_ldT(rows, blk, mult, off)
        if off:
            assert not torch.equal(m, T.pack_map(rows, blk, mult, off, use_off=False))          # row_off ignored lands elsewhere
            assert set(m.tolist()).isdisjoint(T.pack_map(rows, blk, mult, 0).tolist())          # fc1 and gate rows interleave, never meet
    V = 5
    c = T.scatter_case(V, 4, 91)
    want = T.scatter_ref(c, V)
    assert not torch.equal(want, T.scatter_ref(c, V, clamp=False))          # ids -3 and V + 2 wrapped instead of clamped
    assert not torch.equal(want, T.scatter_ref(c, V, accumulate=False))     # duplicates overwritten
    assert torch.equal(want[2], c["table0"][2]) and not torch.equal(want[0], c["table0"][0]) and not torch.equal(want[4], c["table0"][4])
    src = T.bf(T.scaled_rows(5, 8, 93))
    t = T.transpose_ref(src, 5, 8, 64)
    assert t.shape == (8, 64) and torch.equal(t[:, :5], src.T) and not t[:, 5:].any()


# ------------------------------------------------------------------ the size helpers ------------------------------------------------------------------
def test_size_helpers_match_their_restatement():
    lib = hip.lib()
    for (rows, d) in T.LN_STREAM_SHAPES:
        assert lib.ditto_layernorm_bwd_scratch_bytes(rows, 1, d) == T.ln_scratch_bytes(rows, 1, d)
    for (rpg, groups, d) in T.LN_GROUP_SHAPES:
        assert lib.ditto_layernorm_bwd_scratch_bytes(rpg, groups, d) == T.ln_scratch_bytes(rpg, groups, d)
    assert T.ln_chunks(1100, 1) == 69 and T.ln_chunks(300, 70) == 15
    for lens in T.ADALN_LENS:
        for d in T.ADALN_D:
            assert hip.call("ditto_bwd_adaln_packed_scratch_bytes", max_len=max(lens), B=len(lens), d=d) == T.adaln_scratch_bytes(max(lens), len(lens), d)
    for (M, n, _) in T.COLSUM_CASES:
        got = hip.call("ditto_bwd_colsum_scratch_bytes", M=M, n=n)
        assert got == T.colsum_scratch_bytes(M, n) <= 256 * n * 4
    for F in T.GATED_F + [T.GATED_BIG[1]]:
        for M in T.GATED_M:
            assert hip.call("ditto_bwd_colsum_scratch_bytes", M=M, n=2 * F) <= 256 * 2 * F * 4        # the unfused path's second launch fits
    assert T.colsum_chunks(9000, 16) == 256 and (9000 + 255) // 256 == 36                              # four rows in flight: 36 > 32
    assert hip.call("ditto_bwd_colsum_scratch_bytes", M=0, n=8) == 0 and b"ditto_bwd_colsum_scratch_bytes" in lib.ditto_last_error()
    assert hip.call("ditto_bwd_adaln_packed_scratch_bytes", max_len=4, B=1, d=66) == 0 and b"ditto_bwd_adaln_packed" in lib.ditto_last_error()
