"""The forward row kernels of csrc/rowwise.hip at kernel level — ln_kernel's AdaLN modes (dense and packed), the split-K finish with and
without its fused LayerNorm, the text pool / text modulation (dense, variable-length, packed), the time table, the packed row map and the
RoPE tables — against the fp64 references and derived elementwise bounds of rowwise_ref.py, and bitwise wherever the kernels' comments
promise bits.  Every value assertion is elementwise (worst ratio <= 1) or bitwise; `-s` prints one `ROW_RATIO <case> <output> <worst>`
line per case.

Every buffer lies inside a larger allocation with GUARD elements before and after.  What a kernel must not read is NaN (the guards of
every input, the padded text rows, the gaps between split partials); what it must not write carries a fixed bit pattern (the guards of
every output, the other half of xcat at ldraw = 2d, the columns past N at ldo2 / ldu = 2N).  After every launch the patterns are
checked bit for bit and the inputs are bit-identical.  Every index given to a kernel is in range.

Measured on an MI355X (2026-10-19), worst ROW_RATIO per output over all cases: AdaLN h 0.66, u1 0.02 (fp32 h) / 0.006 (bf16 h),
ditto_global_adaln 0.021, the finish's fp32 chain against fp64 0.64 and its fused LayerNorm 0.001, pooled 0.51, tmod 0.014, time table
0.025, RoPE 0.48 (0.39 over the last 64 positions of N = 4099); the table with its reading is in rowwise_ref.py's docstring.  Every
bitwise assertion held: no comment of csrc/rowwise.hip had to be corrected.
"""
import pytest
import torch

import rowwise_ref as R
from ditto_tts_amd import hip
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 4096
PATTERN = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.bfloat16: (torch.int16, 0x7FC5), torch.int32: (torch.int32, -0x5A5A5A5B)}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return hip.lib()


def report(case, what, worst):
    print(f"ROW_RATIO {case} {what} {worst:.3f}")
    assert worst <= 1.0, (case, what, worst)


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.contiguous().view(PATTERN[t.dtype][0] if t.dtype in PATTERN else torch.int64)


class In:
    """a read-only operand inside NaN (floats) / zero (integers) guards; .v is the view the kernel gets"""

    def __init__(self, x):
        x = x.contiguous()
        fill = NAN if x.dtype.is_floating_point else 0
        self.buf = torch.full((x.numel() + 2 * GUARD,), fill, dtype=x.dtype, device=DEV)
        self.buf[GUARD:GUARD + x.numel()] = x.reshape(-1).to(DEV)
        self.v = self.buf[GUARD:GUARD + x.numel()].view(x.shape)
        self.was = self.buf.clone()

    def intact(self):
        return torch.equal(bits(self.buf), bits(self.was))


class Out:
    """an output of `rows` rows of `cols` columns at row stride ld, starting at column col0, inside a buffer that carries the fixed bit
    pattern everywhere; .v is the [rows, cols] view, .p its address; clean() is true when every element outside the view still carries
    the pattern"""

    def __init__(self, rows, cols, dtype, ld=None, col0=0):
        self.rows, self.cols, self.ld, self.col0 = rows, cols, ld or cols, col0
        it, pat = PATTERN[dtype]
        self.buf = torch.full((rows * self.ld + 2 * GUARD,), pat, dtype=it, device=DEV).view(dtype)
        self.image = self.buf[GUARD:GUARD + rows * self.ld].view(rows, self.ld)
        self.v = self.image[:, col0:col0 + cols]
        self.p = self.v.data_ptr()
        self.pat = pat

    def clean(self):
        b = bits(self.buf).clone()
        b[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, self.col0:self.col0 + self.cols] = self.pat
        return bool((b == self.pat).all())


def same_bits(a, b):
    return torch.equal(bits(a), bits(b.to(a.device)))


# =========================================================== AdaLN, dense and packed ===========================================================
ROW_SETS = [("dense", bn) for bn in R.DENSE_ROWS] + [("packed", lens) for lens in R.PACKED_LENS]


def row_map(lib, cu, max_len):
    """(utt, pos) int32 [S] on the device from the row-map entry, guards checked"""
    cu_in = In(torch.tensor(cu, dtype=torch.int32))
    S = cu[-1]
    utt, pos = Out(S, 1, torch.int32), Out(S, 1, torch.int32)
    hip.check(lib.ditto_packed_row_map(cu_in.v.data_ptr(), len(cu) - 1, S, max_len, utt.p, pos.p, stream()))
    torch.cuda.synchronize()
    assert utt.clean() and pos.clean() and cu_in.intact()
    return utt.v.reshape(-1), pos.v.reshape(-1)


def run_adaln(lib, c, ins, kind, use_t=True, h_bf16=False, raw_half=None, u1=False, utt_dev=None, B=None, N=None):
    """one guarded launch; returns dict(h, raw, u1) of device views after the pattern and input checks"""
    M, d = c["x"].shape
    h = Out(M, d, torch.bfloat16 if h_bf16 else torch.float32)
    raw = Out(M, d, torch.bfloat16, ld=2 * d, col0=raw_half * d) if raw_half is not None else None
    uo = Out(M, d, torch.bfloat16) if u1 else None
    t = ins["t"].v.data_ptr() if use_t else None
    g1, be1 = (ptr(ins["g1"].v), ptr(ins["be1"].v)) if u1 else (None, None)
    if kind == "packed":
        hip.check(lib.ditto_adaln_rows_packed(ptr(ins["x"].v), ptr(ins["ttab"].v), ptr(ins["tmod"].v), t, c["steps"], ptr(utt_dev), h.p,
                                              int(h_bf16), raw.p if raw else None, 2 * d, g1, be1, uo.p if uo else None, M, d, stream()))
    else:
        hip.check(lib.ditto_adaln_rows(ptr(ins["x"].v), ptr(ins["ttab"].v), ptr(ins["tmod"].v), t, c["steps"], h.p, int(h_bf16),
                                       raw.p if raw else None, 2 * d, g1, be1, uo.p if uo else None, B, N, d, stream()))
    torch.cuda.synchronize()
    assert h.clean() and (raw is None or raw.clean()) and (uo is None or uo.clean())
    assert all(i.intact() for i in ins.values())
    return dict(h=h.v, raw=raw.v if raw else None, u1=uo.v if uo else None)


def layernorm_launch(lib, x_dev, gamma, beta):
    """ditto_layernorm_bf16 on contiguous fp32 rows: the separate launch the fused paths replace"""
    M, d = x_dev.shape
    xin, g, b = In(x_dev), In(gamma), In(beta)
    o = Out(M, d, torch.bfloat16)
    hip.check(lib.ditto_layernorm_bf16(ptr(xin.v), ptr(g.v), ptr(b.v), o.p, M, d, stream()))
    torch.cuda.synchronize()
    assert o.clean() and xin.intact()
    return o.v


def adaln_inputs(c):
    return {k: In(c[k]) for k in ("x", "ttab", "tmod", "t", "g1", "be1")}


@pytest.mark.parametrize("d", R.ADALN_D)
@pytest.mark.parametrize("rows", ROW_SETS, ids=lambda r: f"{r[0]}{r[1]}".replace(" ", ""))
def test_adaln_every_form_elementwise(lib, rows, d):
    kind, spec = rows
    if kind == "dense":
        B, N = spec
        c = R.adaln_case(R.dense_utt(B, N), d, 11 + d + B)
        utt_dev, lens = None, [N] * B
    else:
        B, N, lens = len(spec), None, spec
        c = R.adaln_case(R.packed_utt(spec), d, 23 + d + spec[0])
        cu = [0] + torch.tensor(spec).cumsum(0).tolist()
        utt_dev, _ = row_map(lib, cu, max(spec))
        assert torch.equal(utt_dev.cpu(), c["utt"])
    case = f"adaln_{kind}{spec}_d{d}".replace(" ", "")
    ins = adaln_inputs(c)
    worst = {}
    full = None
    for use_t in (True, False):
        h64, hb = R.adaln_ref(c, use_t)
        for h_bf16 in (False, True):
            for raw_half in (None, 0, 1):
                for u1 in (False, True):
                    got = run_adaln(lib, c, ins, kind, use_t, h_bf16, raw_half, u1, utt_dev, B, N)
                    r = dict(h=R.worst_ratio(got["h"].float().cpu(), h64, hb, "bf16" if h_bf16 else None))
                    if raw_half is not None:
                        assert same_bits(got["raw"], c["x"].to(torch.bfloat16)), (case, "raw copy is not bf16(x)")
                    if u1:
                        if h_bf16:
                            u, ub = R.u1_ref_bf16_stream(h64, hb, c["g1"], c["be1"])
                            r["u1_bf16_stream"] = R.worst_ratio(got["u1"].float().cpu(), u, ub, "bf16")
                        else:
                            u, ub = R.u1_ref(got["h"].cpu(), c["g1"], c["be1"])
                            r["u1"] = R.worst_ratio(got["u1"].float().cpu(), u, ub, "bf16")
                            # the fused norm1 is the separate launch, bit for bit
                            assert same_bits(got["u1"], layernorm_launch(lib, got["h"], c["g1"], c["be1"])), (case, "u1 != LayerNorm launch")
                    for k, v in r.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                        assert v <= 1.0, (case, use_t, h_bf16, raw_half, u1, k, v)
                    if use_t and not h_bf16 and raw_half == 1 and u1:
                        full = got
    for k, v in worst.items():
        report(case, k, v)
    # an utterance's rows are the same bits alone (a dense launch of its own) and among its neighbours (dense or packed)
    r0 = 0
    for b, n in enumerate(lens):
        alone = dict(c, x=c["x"][r0:r0 + n], tmod=c["tmod"][b:b + 1], t=c["t"][b:b + 1], utt=torch.zeros(n, dtype=torch.int32))
        got = run_adaln(lib, alone, adaln_inputs(alone), "dense", True, False, 1, True, None, 1, n)
        for k in ("h", "raw", "u1"):
            assert same_bits(got[k], full[k][r0:r0 + n]), (case, "utterance", b, k, "differs alone")
        r0 += n


@pytest.mark.parametrize("d", R.ADALN_D)
def test_global_adaln_module_null_t_form(lib, d):
    """ditto_global_adaln: the two modulation launches, then the AdaLN kernel with t == NULL (the table row is the batch index)"""
    B, N, T, td, dt = 3, 5, 4, 96, 80
    c = R.adaln_case(R.dense_utt(B, N), d, 77 + d)
    k = R.cond_case(T, dt, d, 5 + d)
    text = torch.nan_to_num(k["text"], nan=0.25)
    temb = R.asym((B, td), 9 + d).float()
    tw = (R.asym((2 * d, td), 10 + d) / td ** 0.5).float()
    tb = (0.1 * R.asym((2 * d,), 11 + d)).float()
    full = torch.tensor([T] * B, dtype=torch.int32)
    _, _, mt, emt, _ = R.text_mod_ref(dict(text=temb[:, None, :], lens=torch.ones(B, dtype=torch.int32), wx=tw, bx=tb))
    _, _, mx, emx, _ = R.text_mod_ref(dict(text=text, lens=full, wx=k["wx"], bx=k["bx"]))
    h64, hb = R.adaln_ref(dict(c, ttab=mt, tmod=mx), use_t=False, e_ttab=emt, e_tmod=emx)
    ins = [In(v) for v in (c["x"], temb, text, tw, tb, k["wx"], k["bx"])]
    out = Out(B * N, d, torch.float32)
    nb = lib.ditto_global_adaln_scratch_bytes(B, d, td, dt)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    hip.check(lib.ditto_global_adaln(*[i.v.data_ptr() for i in ins], B, N, T, d, td, dt, out.p, scratch.data_ptr(), nb, stream()))
    torch.cuda.synchronize()
    assert out.clean() and all(i.intact() for i in ins)
    report(f"global_adaln_d{d}", "h", R.worst_ratio(out.v.cpu(), h64, hb))


# ================================================================ split-K finish ================================================================
def run_finish(lib, f, nsplit, stride, bias, res, ldo2, ldu):
    """one guarded launch; res: None / "given" / "alias"; ldo2 / ldu 0: that output absent.  Returns (out, out2, u) device views"""
    M, N = f["p"].shape[1:]
    pbuf = torch.full((nsplit, stride), NAN)
    pbuf[:, :M * N] = f["p"].reshape(nsplit, -1)
    pin = In(pbuf.reshape(-1)[:(nsplit - 1) * stride + M * N])
    ins = [pin]
    b_in = g_in = e_in = r_in = None
    if bias:
        b_in = In(f["bias"]); ins.append(b_in)
    out = Out(M, N, torch.float32)
    rp = None
    if res == "given":
        r_in = In(f["res"]); ins.append(r_in); rp = ptr(r_in.v)
    elif res == "alias":
        out.v.copy_(f["res"].to(DEV)); rp = out.p
    o2 = Out(M, N, torch.bfloat16, ld=ldo2) if ldo2 else None
    u = Out(M, N, torch.bfloat16, ld=ldu) if ldu else None
    if ldu:
        g_in, e_in = In(f["gamma"]), In(f["beta"]); ins += [g_in, e_in]
    hip.check(lib.ditto_splitk_finish(ptr(pin.v), nsplit, stride, ptr(b_in.v) if bias else None, rp, out.p, o2.p if o2 else None, ldo2,
                                      ptr(g_in.v) if ldu else None, ptr(e_in.v) if ldu else None, u.p if u else None, ldu, M, N, stream()))
    torch.cuda.synchronize()
    assert out.clean() and (o2 is None or o2.clean()) and (u is None or u.clean()) and all(i.intact() for i in ins)
    return out.v, o2.v if o2 else None, u.v if u else None


@pytest.mark.parametrize("nsplit", R.FINISH_NSPLIT)
@pytest.mark.parametrize("shape", R.FINISH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_splitk_finish_bitwise_and_fused_layernorm(lib, shape, nsplit):
    M, N = shape
    f = R.finish_case(M, N, nsplit, 31 + M + nsplit)
    case = f"finish_{M}x{N}_s{nsplit}"
    worst_u = worst_out = 0.0
    for bias in (False, True):
        for res in (None, "given", "alias"):
            chain = R.finish_chain(f["p"], f["bias"] if bias else None, f["res"] if res else None)
            o64, oe = R.finish_ref(f["p"], f["bias"] if bias else None, f["res"] if res else None)
            worst_out = max(worst_out, R.worst_ratio(chain, o64, oe))
            u64, ue = R.u1_ref(chain, f["gamma"], f["beta"])
            u_two = None
            for stride in (M * N, M * N + 64):
                for ldo2 in (0, N, 2 * N):
                    for ldu in (0, N, 2 * N):
                        out, o2, u = run_finish(lib, f, nsplit, stride, bias, res, ldo2, ldu)
                        tag = (case, bias, res, stride, ldo2, ldu)
                        assert same_bits(out, chain), (tag, "out is not the fp32 chain")
                        if o2 is not None:
                            assert same_bits(o2, chain.to(torch.bfloat16)), (tag, "out2 is not bf16(out)")
                        if u is not None:
                            if u_two is None:      # the plain finish's out (bitwise the chain, asserted above) through the LayerNorm launch
                                u_two = layernorm_launch(lib, chain.to(DEV), f["gamma"], f["beta"]).clone()
                            assert same_bits(u, u_two), (tag, "fused u differs from finish + LayerNorm launch")
                            r = R.worst_ratio(u.float().cpu(), u64, ue, "bf16")
                            worst_u = max(worst_u, r)
                            assert r <= 1.0, (tag, r)
    report(case, "out_chain_vs_fp64", worst_out)
    report(case, "u", worst_u)


# ================================================================= conditioning =================================================================
def run_text_mod(lib, form, text, lens_or_cu, c, B, T, dt, d):
    tin, win, bin_ = In(text), In(c["wx"]), In(c["bx"])
    lin = In(lens_or_cu) if lens_or_cu is not None else None
    pooled, tmod = Out(B, dt, torch.float32), Out(B, 2 * d, torch.float32)
    if form == "packed":
        hip.check(lib.ditto_text_mod_packed(ptr(tin.v), ptr(lin.v), text.shape[0], T, ptr(win.v), ptr(bin_.v), pooled.p, tmod.p, B, dt, d,
                                            stream()))
    else:
        hip.check(lib.ditto_text_mod(ptr(tin.v), ptr(lin.v) if lin else None, ptr(win.v), ptr(bin_.v), pooled.p, tmod.p, B, T, dt, d,
                                     stream()))
    torch.cuda.synchronize()
    assert pooled.clean() and tmod.clean() and tin.intact() and win.intact() and bin_.intact()
    return pooled.v, tmod.v


@pytest.mark.parametrize("dims", R.COND_DIMS, ids=lambda s: f"dt{s[0]}_d{s[1]}")
@pytest.mark.parametrize("T", R.COND_T)
def test_text_pool_and_modulation(lib, T, dims):
    dt, d = dims
    c = R.cond_case(T, dt, d, 41 + T + dt)
    case = f"textmod_T{T}_dt{dt}_d{d}"
    p64, ep, t64, et, floor = R.text_mod_ref(c)
    pv, tv = run_text_mod(lib, "varlen", c["text"], c["lens"], c, 3, T, dt, d)
    report(case, "pooled", R.worst_ratio(pv.cpu(), p64, ep))
    report(case, "tmod", R.worst_ratio(tv.cpu(), t64, et))
    pp, tp = run_text_mod(lib, "packed", c["packed"], c["cu"], c, 3, T, dt, d)
    assert same_bits(pp, pv) and same_bits(tp, tv), (case, "packed differs from variable-length")
    for b, n in enumerate(c["lens"].tolist()):
        pa, ta = run_text_mod(lib, "dense", c["text"][b:b + 1, :n], None, c, 1, n, dt, d)
        assert same_bits(pa, pv[b:b + 1]) and same_bits(ta, tv[b:b + 1]), (case, "utterance", b, "differs alone (dense, T = T_b)")


@pytest.mark.parametrize("td", R.TIME_TD)
def test_time_table(lib, td):
    d, steps = 64, 3
    c = R.time_case(td, d, 3 + td, steps)
    want, e, floor = R.time_table_ref(c)
    ins = [In(c[k]) for k in ("emb", "w0", "b0", "w2", "b2", "wt", "bt")]
    out = Out(steps, 2 * d, torch.float32)
    hip.check(lib.ditto_time_table(*[i.v.data_ptr() for i in ins], out.p, steps, td, d, stream()))
    torch.cuda.synchronize()
    assert out.clean() and all(i.intact() for i in ins)
    report(f"time_table_td{td}", "ttab", R.worst_ratio(out.v.cpu(), want, e))


# ================================================================== packed row map ==================================================================
@pytest.mark.parametrize("name", list(R.ROW_MAPS))
def test_packed_row_map_exact(lib, name):
    cu = R.ROW_MAPS[name]
    longest = max(b - a for a, b in zip(cu, cu[1:]))
    for max_len in (longest, max(1, longest - 2)):         # below the longest: the documented clamp of pos
        utt, pos = row_map(lib, cu, max_len)
        wu, wp = R.row_map_ref(cu, max_len)
        assert torch.equal(utt.cpu(), wu) and torch.equal(pos.cpu(), wp), (name, max_len)


# ==================================================================== RoPE tables ====================================================================
@pytest.fixture(scope="module")
def rope_engine():
    from ditto_tts_amd.config import DiTTOConfig
    from ditto_tts_amd.engine import DenoiseEngine
    from ditto_tts_amd.synth import synthetic_state_dict
    cfg = DiTTOConfig(256, 1, 4, 64, 256, 4)            # head_dim 64: half = 32, the model's inv_freq
    sd = synthetic_state_dict(cfg, seed=1)
    assert torch.equal(sd["rotary.inv_freq"], R.inv_freq())
    return DenoiseEngine(cfg, sd)


@pytest.mark.parametrize("N", R.ROPE_N)
def test_rope_tables_to_the_far_end(lib, rope_engine, N):
    half = 32
    c64, s64, e, floor = R.rope_ref(N, R.inv_freq())
    co, so = Out(N, half, torch.float32), Out(N, half, torch.float32)
    hip.check(lib.ditto_rope_tables(rope_engine.handle, N, co.p, so.p, stream()))
    torch.cuda.synchronize()
    assert co.clean() and so.clean()
    cg, sg = co.v.cpu(), so.v.cpu()
    report(f"rope_N{N}", "cos", R.worst_ratio(cg, c64, e))
    report(f"rope_N{N}", "sin", R.worst_ratio(sg, s64, e))
    last = slice(max(0, N - 64), N)                        # the far end on its own: the worst case is reported, not averaged away
    report(f"rope_N{N}", "cos_last64", R.worst_ratio(cg[last], c64[last], e[last]))
    report(f"rope_N{N}", "sin_last64", R.worst_ratio(sg[last], s64[last], e[last]))
