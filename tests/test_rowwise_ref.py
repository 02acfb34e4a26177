"""rowwise_ref.py without a GPU: the fp64 references against torch's own operators on the shapes test_gpu_rowwise.py runs, the fp32
emulation of every kernel inside every bound with no case excluded, and a table of the defects a wrong kernel could have — each applied
to the emulation on the GPU tests' own inputs and each caught by the bound or by the exact comparison the GPU test makes.  That table is
what shows the small shapes and the data are discriminating."""
import numpy as np
import pytest
import torch

import rowwise_ref as R
from ditto_tts_amd import hip

D_SMALL = [64, 772]                       # the mutation table runs where the GPU test crosses every output form


def adaln_cases(ds=R.ADALN_D):
    for d in ds:
        for B, N in R.DENSE_ROWS:
            yield f"dense{B}x{N}_d{d}", R.adaln_case(R.dense_utt(B, N), d, 11 + d + B)
        for lens in R.PACKED_LENS:
            yield f"packed{lens}_d{d}", R.adaln_case(R.packed_utt(lens), d, 23 + d + lens[0])


# ------------------------------------------------------------ references against torch ------------------------------------------------------------
def test_references_agree_with_torch():
    """every reference against torch's own fp64 operators (relative 1e-11 of the row's scale), and torch's fp32 operators within the
    bound, on every shape the GPU test runs"""
    fn = torch.nn.functional
    close = lambda a, b: torch.allclose(a, b, rtol=1e-11, atol=1e-11 * float(b.abs().max()))
    for name, c in adaln_cases():
        d = c["x"].shape[1]
        h, hb = R.adaln_ref(c)
        b = c["utt"].long()
        tt, tm = c["ttab"].double()[c["t"][b]], c["tmod"].double()[b]
        ln = fn.layer_norm(c["x"].double(), (d,), eps=1e-5)
        assert close(h, ln * (1 + tt[:, :d] + tm[:, :d]) + tt[:, d:] + tm[:, d:]), name
        ln32 = fn.layer_norm(c["x"], (d,), eps=1e-5)
        h32 = ln32 * (1 + c["ttab"][c["t"][b], :d] + c["tmod"][b, :d]) + c["ttab"][c["t"][b], d:] + c["tmod"][b, d:]
        assert R.worst_ratio(h32, h, hb) <= 1.0, name
        u, ue = R.u1_ref(h32, c["g1"], c["be1"])
        assert close(u, fn.layer_norm(h32.double(), (d,), c["g1"].double(), c["be1"].double(), 1e-5)), name
        assert R.worst_ratio(fn.layer_norm(h32, (d,), c["g1"], c["be1"], 1e-5).to(torch.bfloat16).float(), u, ue, "bf16") <= 1.0, name
    for M, N, ns, f in finish_cases():
        out, _ = R.finish_ref(f["p"], f["bias"], f["res"])
        chain = R.finish_chain(f["p"], f["bias"], f["res"])
        assert close(out, (f["p"].double().sum(0) + f["bias"].double()) + f["res"].double())
        assert chain.dtype == torch.float32
        want32 = f["p"][0]
        for s in range(1, ns):
            want32 = torch.add(want32, f["p"][s])
        assert torch.equal(chain, torch.add(torch.add(want32, f["bias"]), f["res"]))
    for T, dt, d, k in cond_cases():
        p, ep, tmod, et, _ = R.text_mod_ref(k)
        for bb, n in enumerate(k["lens"]):
            rows = k["text"][bb, :int(n)]
            assert close(p[bb], rows.double().mean(0))
            assert close(tmod[bb], fn.linear(fn.silu(rows.double().mean(0)), k["wx"].double(), k["bx"].double()))
            assert R.worst_ratio(rows.mean(0), p[bb], ep[bb]) <= 1.0
            assert R.worst_ratio(fn.linear(fn.silu(rows.mean(0)), k["wx"], k["bx"]), tmod[bb], et[bb]) <= 1.0
    for td in R.TIME_TD:
        tc = R.time_case(td, 64, 3 + td)
        tab, te, _ = R.time_table_ref(tc)
        dd = {kk: v.double() for kk, v in tc.items()}
        silu, lin = fn.silu, fn.linear
        assert close(tab, lin(silu(lin(silu(lin(dd["emb"], dd["w0"], dd["b0"])), dd["w2"], dd["b2"])), dd["wt"], dd["bt"]))
        assert R.worst_ratio(lin(silu(lin(silu(lin(tc["emb"], tc["w0"], tc["b0"])), tc["w2"], tc["b2"])), tc["wt"], tc["bt"]), tab, te) <= 1.0
    for name, cu in R.ROW_MAPS.items():
        utt, pos = R.row_map_ref(cu, 5)
        for r in range(cu[-1]):
            b = max(i for i in range(len(cu) - 1) if cu[i] <= r)
            assert int(utt[r]) == b and int(pos[r]) == min(r - cu[b], 4), (name, r)
    cu = R.ROW_MAPS["zero_len"]
    utt, pos = R.row_map_ref(cu, 12)
    assert utt.tolist() == [0] * 3 + [2] * 4 + [3] + [4] * 12 and pos.tolist() == [0, 1, 2, 0, 1, 2, 3, 0] + list(range(12))
    invf = R.inv_freq()
    cs, sn, _, _ = R.rope_ref(5, invf)
    want = torch.arange(5, dtype=torch.float32)[:, None] * invf[None, :]
    assert torch.equal(cs, torch.cos(want.double())) and torch.equal(sn, torch.sin(want.double()))


# ------------------------------------------------------------------- the emulation -------------------------------------------------------------------
def adaln_ratios(c, emu, use_t=True, h_bf16=False):
    """worst ratio of each output of an AdaLN launch (emulated or real) to its bound: dict(h, raw, u1); raw is 0 / inf (bitwise)"""
    h64, hb = R.adaln_ref(c, use_t)
    out = dict(h=R.worst_ratio(emu["h"].float(), h64, hb, "bf16" if h_bf16 else None))
    if emu.get("raw") is not None:
        out["raw"] = 0.0 if torch.equal(R.bf16_bits(emu["raw"]), R.bf16_bits(c["x"].to(torch.bfloat16))) else float("inf")
    if emu.get("u1") is not None:
        if h_bf16:
            u, ub = R.u1_ref_bf16_stream(h64, hb, c["g1"], c["be1"])
        else:
            u, ub = R.u1_ref(emu["h"], c["g1"], c["be1"])
        out["u1"] = R.worst_ratio(emu["u1"].float(), u, ub, "bf16")
    return out


def test_unmutated_adaln_emulation_is_inside_every_bound():
    worst = {}
    for name, c in adaln_cases():
        for use_t in (True, False):
            if not use_t and int(c["utt"].max()) >= c["steps"]:
                continue
            for h_bf16 in (False, True):
                for k, v in adaln_ratios(c, R.adaln_emulate(c, use_t, h_bf16), use_t, h_bf16).items():
                    worst[k] = max(worst.get(k, 0.0), v)
                    assert v <= 1.0, (name, use_t, h_bf16, k, v)
    print("emulation worst ratios (AdaLN):", worst)


def finish_cases():
    for M, N in R.FINISH_SHAPES:
        for ns in R.FINISH_NSPLIT:
            yield M, N, ns, R.finish_case(M, N, ns, 31 + M + ns)


def test_unmutated_finish_emulation_is_inside_every_bound():
    for M, N, ns, f in finish_cases():
        for bias in (None, f["bias"]):
            for res in (None, f["res"]):
                chain = R.finish_chain(f["p"], bias, res)
                out, e = R.finish_ref(f["p"], bias, res)
                assert R.worst_ratio(chain, out, e) <= 1.0, (M, N, ns)
                u, ue = R.u1_ref(chain, f["gamma"], f["beta"])
                assert R.worst_ratio(R.layernorm_emulate(chain, f["gamma"], f["beta"]).float(), u, ue, "bf16") <= 1.0, (M, N, ns)
                assert torch.equal(R.out2_image(chain, 2 * N, 7.0)[:, :N], chain.to(torch.bfloat16))


def cond_cases():
    for T in R.COND_T:
        for dt, d in R.COND_DIMS:
            yield T, dt, d, R.cond_case(T, dt, d, 41 + T + dt)


def cond_ratios(c, pooled, tmod):
    p, ep, tm, et, _ = R.text_mod_ref(c)
    return R.worst_ratio(pooled, p, ep), R.worst_ratio(tmod, tm, et)


def test_unmutated_conditioning_emulation_is_inside_every_bound():
    floors = []
    for T, dt, d, c in cond_cases():
        starts = [b * T for b in range(3)]
        pooled = R.pool_emulate(c["text"].reshape(-1, dt), starts, c["lens"])
        packed = R.pool_emulate(c["packed"], c["cu"][:-1], c["lens"])
        assert torch.equal(pooled, packed)
        rp, rt = cond_ratios(c, pooled, R.text_mod_emulate(pooled, c["wx"], c["bx"]))
        assert rp <= 1.0 and rt <= 1.0, (T, dt, d, rp, rt)
        floors.append(R.text_mod_ref(c)[4])
    tf = []
    for td in R.TIME_TD:
        tc = R.time_case(td, 64, 3 + td)
        out, e, floor = R.time_table_ref(tc)
        assert R.worst_ratio(R.time_table_emulate(tc), out, e) <= 1.0, td
        tf.append(floor)
    print(f"silu floors: text modulation {max(floors):.3e}, time table {max(tf):.3e}")
    assert 2.0 ** -26 < max(floors) < 2.0 ** -21 and 2.0 ** -26 < max(tf) < 2.0 ** -21      # a floor of about one fp32 ulp


def test_unmutated_rope_emulation_is_inside_the_bound():
    invf = R.inv_freq()
    for N in R.ROPE_N:
        c, s, e, floor = R.rope_ref(N, invf)
        ang = R.rope_angles(N, invf)
        assert R.worst_ratio(torch.cos(ang), c, e) <= 1.0 and R.worst_ratio(torch.sin(ang), s, e) <= 1.0
        print(f"cos / sin floor at N = {N}: {floor:.3e}")
        assert floor <= 2.0 ** -23


# ------------------------------------------------------------------ the mutation table ------------------------------------------------------------------
ADALN_MUTANTS = ["block_utt", "swap_halves", "no_one", "t_is_b", "unbiased", "no_eps", "u1_stats_of_x", "u1_from_bf16_h"]


@pytest.mark.parametrize("mutant", ADALN_MUTANTS)
def test_adaln_mutant_is_caught(mutant):
    """caught = some output of some case of the GPU test leaves its bound.  (1, 1) rows cannot show a misassigned row, eps only shows
    on a row of small variance: the table is judged over the case set, as the GPU test is."""
    caught = []
    for name, c in adaln_cases(D_SMALL):
        for h_bf16 in (False, True):
            r = adaln_ratios(c, R.adaln_emulate(c, True, h_bf16, mutate=mutant), True, h_bf16)
            if max(r.values()) > 1.0:
                caught.append((name, h_bf16))
    assert caught, mutant
    if mutant == "block_utt":        # the straddling case of the issue, dense and packed, by name
        assert any(n.startswith("dense3x5") for n, _ in caught) and any(n.startswith("packed[1, 6, 3]") for n, _ in caught)
    if mutant in ("u1_stats_of_x", "u1_from_bf16_h"):      # visible in both stream types
        assert {hb for _, hb in caught} == {False, True}, (mutant, caught)


@pytest.mark.parametrize("mutant", ["drop_last_split", "bias_flat_index"])
def test_finish_mutant_breaks_the_bitwise_chain(mutant):
    caught = 0
    for M, N, ns, f in finish_cases():
        good, bad = R.finish_chain(f["p"], f["bias"], f["res"]), R.finish_chain(f["p"], f["bias"], f["res"], mutate=mutant)
        caught += not torch.equal(good.view(torch.int32), bad.view(torch.int32))
    assert caught >= (8 if mutant == "drop_last_split" else 9)     # every nsplit > 1 / every M > 1 case


def test_out2_stride_mutant_breaks_the_image():
    for M, N, ns, f in finish_cases():
        chain = R.finish_chain(f["p"], f["bias"], f["res"])
        same = torch.equal(R.bf16_bits(R.out2_image(chain, 2 * N, 7.0)), R.bf16_bits(R.out2_image(chain, 2 * N, 7.0, mutate="out2_stride_n")))
        assert same == (M == 1), (M, N)


@pytest.mark.parametrize("mutant", ["divide_by_T", "one_row_past", "packed_from_next_offset"])
def test_pool_mutant_is_caught(mutant):
    caught = 0
    for T, dt, d, c in cond_cases():
        if mutant == "packed_from_next_offset":
            flat = torch.cat([c["packed"], torch.full((T + 1, dt), float("nan"))])          # what lies past the buffer: the guard
            pooled = R.pool_emulate(flat, c["cu"][:-1], c["lens"], mutate=mutant)
        else:
            flat = torch.cat([c["text"].reshape(-1, dt), torch.full((1, dt), float("nan"))])
            pooled = R.pool_emulate(flat, [b * T for b in range(3)], c["lens"], T_div=T, mutate=mutant)
        rp, rt = cond_ratios(c, pooled, R.text_mod_emulate(pooled, c["wx"], c["bx"]))
        caught += rp > 1.0 and rt > 1.0
    assert caught >= (12 if mutant == "divide_by_T" else 15)        # divide_by_T needs an utterance shorter than T: every T > 1


@pytest.mark.parametrize("mutant", ["silu_missing", "bias_of_next_row"])
def test_text_modulation_mutant_is_caught(mutant):
    """beyond the issue's table: tmod's bound is dominated by its dot-product term (measured ratio 0.014), so show that it still
    refuses a wrong modulation on every case"""
    for T, dt, d, c in cond_cases():
        pooled = R.pool_emulate(c["packed"], c["cu"][:-1], c["lens"])
        rp, rt = cond_ratios(c, pooled, R.text_mod_emulate(pooled, c["wx"], c["bx"], mutate=mutant))
        assert rp <= 1.0 < rt, (mutant, T, dt, d, rt)


@pytest.mark.parametrize("mutant", ["embedding_of_next_step", "second_silu_missing"])
def test_time_table_mutant_is_caught(mutant):
    for td in R.TIME_TD:
        tc = R.time_case(td, 64, 3 + td)
        out, e, _ = R.time_table_ref(tc)
        assert R.worst_ratio(R.time_table_emulate(tc, mutate=mutant), out, e) > 1.0, (mutant, td)


@pytest.mark.parametrize("mutant", ["start_row_to_previous", "zero_length_claims"])
def test_row_map_mutant_is_caught(mutant):
    hit = []
    for name, cu in R.ROW_MAPS.items():
        ml = int(np.diff(cu).max())
        good, bad = R.row_map_ref(cu, ml), R.row_map_ref(cu, ml, mutate=mutant)
        if not (torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1])):
            hit.append(name)
    assert "zero_len" in hit and (mutant == "zero_length_claims" or "two_blocks" in hit), hit


def test_rope_flat_index_mutant_is_caught():
    invf = R.inv_freq()
    for N in R.ROPE_N[1:]:
        c, s, e, _ = R.rope_ref(N, invf)
        ang = R.rope_angles(N, invf, mutate="angle_from_flat_index")
        assert R.worst_ratio(torch.cos(ang), c, e) > 1.0 and R.worst_ratio(torch.sin(ang), s, e) > 1.0


# ------------------------------------------------------------------ the entries' checks ------------------------------------------------------------------
def test_row_entries_refuse_what_they_cannot_serve():
    """host-side validation only: nothing is launched (every call fails before it), so fake aligned addresses are enough"""
    lib = hip.lib()
    P, ODD = 0x10000, 0x10004
    ok_adaln = lambda **k: [k.get("x", P), P, P, k.get("t", P), k.get("steps", 7), P, 0, k.get("raw", None), k.get("ldraw", 0),
                            k.get("g1", None), None, k.get("u1", None), k.get("B", 1), 1, k.get("d", 64), None]
    assert lib.ditto_adaln_rows(*ok_adaln(d=66)) == hip.ERR_SHAPE
    assert lib.ditto_adaln_rows(*ok_adaln(d=2052)) == hip.ERR_SHAPE
    assert lib.ditto_adaln_rows(*ok_adaln(B=0)) == hip.ERR_SHAPE
    assert lib.ditto_adaln_rows(*ok_adaln(steps=0)) == hip.ERR_SHAPE
    assert lib.ditto_adaln_rows(*ok_adaln(raw=P, ldraw=60)) == hip.ERR_SHAPE
    assert lib.ditto_adaln_rows(*ok_adaln(raw=P, ldraw=66)) == hip.ERR_SHAPE
    assert lib.ditto_adaln_rows(*ok_adaln(u1=P)) == hip.ERR_ARG and b"g1" in lib.ditto_last_error()
    assert lib.ditto_adaln_rows(*ok_adaln(x=ODD)) == hip.ERR_ARG and b"aligned" in lib.ditto_last_error()
    assert lib.ditto_adaln_rows_packed(P, P, P, P, 7, None, P, 0, None, 0, None, None, None, 4, 64, None) == hip.ERR_ARG
    assert lib.ditto_adaln_rows_packed(P, P, P, P, 7, P, P, 0, None, 0, None, None, None, 0, 64, None) == hip.ERR_SHAPE
    fin = lambda **k: [P, k.get("ns", 2), k.get("stride", 4 * 64), None, None, P, k.get("o2", None), k.get("ldo2", 0), k.get("g", None),
                       k.get("g", None), k.get("u", None), k.get("ldu", 0), 4, k.get("N", 64), None]
    assert lib.ditto_splitk_finish(*fin(N=66)) == hip.ERR_SHAPE
    assert lib.ditto_splitk_finish(*fin(ns=0)) == hip.ERR_SHAPE
    assert lib.ditto_splitk_finish(*fin(stride=4 * 64 - 4)) == hip.ERR_SHAPE
    assert lib.ditto_splitk_finish(*fin(stride=4 * 64 + 2)) == hip.ERR_SHAPE
    assert lib.ditto_splitk_finish(*fin(o2=P, ldo2=60)) == hip.ERR_SHAPE
    assert lib.ditto_splitk_finish(*fin(u=P, ldu=64)) == hip.ERR_ARG and b"gamma" in lib.ditto_last_error()
    assert lib.ditto_splitk_finish(*fin(u=P, g=P, ldu=62)) == hip.ERR_SHAPE
    assert lib.ditto_splitk_finish(*fin(u=P, g=P, ldu=4096, N=2052, stride=4 * 2052)) == hip.ERR_SHAPE
    assert lib.ditto_text_mod(P, None, P, P, P, P, 3, 0, 64, 64, None) == hip.ERR_SHAPE
    assert lib.ditto_text_mod_packed(P, P, 0, 4, P, P, P, P, 3, 64, 64, None) == hip.ERR_SHAPE
    assert lib.ditto_time_table(P, P, P, P, P, P, P, P, 3, 5000, 64, None) == hip.ERR_SHAPE
    assert lib.ditto_time_table(P, P, P, P, P, P, P, P, 0, 32, 64, None) == hip.ERR_SHAPE
    assert lib.ditto_packed_row_map(P, 3, 9, 0, P, P, None) == hip.ERR_SHAPE
