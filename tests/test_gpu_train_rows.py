"""The backward pass's row kernels (csrc/train.hip, csrc/train_packed.hip) one launch at a time through the entries of
include/ditto_train_rows.h — LayerNorm backward in its three residual-stream forms and its group form, the per-utterance GlobalAdaLN
reduction, the gated-MLP derivative with and without its fused bias sums, the two-stage column sums and their finish kernels, the batched
bf16 transpose, the dropout softmax rows forward and backward, the three small-linear kernels, the embedding scatter-add and the packed-order
packers and unpackers — against the fp64 references and derived elementwise bounds of train_rows_ref.py, and bitwise wherever the kernels'
comments promise bits ("bit-reproducible gradients": every deterministic pair is run twice).  Every value assertion is elementwise (worst
ratio <= 1) or bitwise; `-s` prints one `TROW_RATIO <case> <output> <worst>` line per assertion.

Every buffer lies inside a larger allocation with GUARD elements before and after: NaN where nothing may be read (the guards of every
input, the columns past n of a strided operand, the padding columns of the scores), a fixed bit pattern where nothing may be written (the
guards of every output, the positions of a packed destination that the row map never reaches).  Patterns and inputs are checked bit for
bit after every launch.  The byte sizes given to the entries are those of the views, not of the allocations, and the entries are called
through hip.call by parameter name only.  A launch the HIP runtime refuses, or a device fault at the synchronisation behind it, ends the
session: nothing more is started on that GPU.

Measured on an MI355X (2026-10-20): every case inside its bound, worst TROW_RATIO 0.883 (LayerNorm dx_accum: the accumulator's own
rounding) — the table per output is in train_rows_ref.py's docstring; the whole file runs in under ten seconds.
"""
import math

import pytest
import torch

import train_rows_ref as T
from ditto_tts_amd import hip
from gemm_epi_ref import worst_ratio
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 4096
PATTERN = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.bfloat16: (torch.int16, 0x7FC5), torch.int32: (torch.int32, -0x5A5A5A5B),
           torch.uint8: (torch.uint8, 0xA5)}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64, torch.uint8: torch.uint8}
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return hip.lib()


def report(case, what, worst):
    print(f"TROW_RATIO {case} {what} {worst:.3f}")
    assert worst <= 1.0, (case, what, worst)


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


class In:
    """a read-only operand inside NaN (floats) / zero (integers) guards, `shift` elements off the allocation's alignment; .v is the view
    the kernel gets, .p its address, .nbytes its size: the flat extent of the tensor given (NaN inside it = never to be read)"""

    def __init__(self, x, shift=0):
        x = x.contiguous()
        fill = NAN if x.dtype.is_floating_point else 0
        self.buf = torch.full((x.numel() + 2 * GUARD + shift,), fill, dtype=x.dtype, device=DEV)
        self.v = self.buf[GUARD + shift:GUARD + shift + x.numel()]
        self.v.copy_(x.reshape(-1))
        self.v = self.v.view(x.shape)
        self.p, self.nbytes = self.v.data_ptr(), x.numel() * x.element_size()
        self.was = self.buf.clone()

    def intact(self):
        return torch.equal(bits(self.buf), bits(self.was))


class Out:
    """`numel` elements that a kernel may write inside a buffer that carries the fixed bit pattern; init: what stands there before the
    launch (an accumulator) instead of the pattern.  clean(): every guard element still carries the pattern.  untouched(mask): so do
    the elements of the view where mask is False."""

    def __init__(self, shape, dtype, init=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        it, self.pat = PATTERN[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.pat, dtype=it, device=DEV).view(dtype)
        self.v = self.buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.v.copy_(init)
        self.p, self.nbytes, self.n = self.v.data_ptr(), n * self.v.element_size(), n

    def clean(self):
        b = bits(self.buf)
        return bool((b[:GUARD] == self.pat).all()) and bool((b[GUARD + self.n:] == self.pat).all())

    def untouched(self, written):
        return bool((bits(self.v)[~written.to(DEV)] == self.pat).all())

    def cpu(self):
        return self.v.detach().cpu()


def scratch(nbytes):
    return Out(max(nbytes // 4, 1), F32)


def launch(name, ins, outs, **kw):
    """one entry by parameter names; then every guard pattern and every input bit for bit"""
    rc = hip.call(name, stream=stream(), **kw)
    if rc == hip.ERR_HIP:
        pytest.exit(f"{name}: the HIP runtime refused the launch ({hip.lib().ditto_last_error().decode()}): nothing more is started", 3)
    assert rc == hip.OK, (name, rc, hip.lib().ditto_last_error().decode())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                      # a fault on the device: no further launch in this session
        pytest.exit(f"{name}: {e}", 3)
    assert all(o.clean() for o in outs if o is not None), name
    assert all(i.intact() for i in ins if i is not None), name


def pb(prefix, box):
    """the pointer and byte size of a box (or NULL) as the two keyword arguments"""
    return {prefix: None if box is None else box.p, prefix + "_bytes": 0 if box is None else box.nbytes}


# =========================================================== LayerNorm backward ===========================================================
def ln_stream_launch(c, form, gamma, dests, colsum):
    rows, d = c["x"].shape
    dy, x, g = In(c["dy"]), In(c["x"]), In(c["gamma"]) if gamma else None
    acc, dxb = Out((rows, d), F32, init=c["acc0"]), Out((rows, d), BF16)
    dg, db = (Out(d, F32), Out(d, F32)) if dests else (None, None)
    cs = Out(d, F32) if colsum else None
    sc = scratch(T.ln_scratch_bytes(rows, 1, d))
    launch("ditto_bwd_ln_stream", [dy, x, g], [acc, dxb, dg, db, cs, sc], **pb("dy", dy), dy_bf16=int(form[0] == "bf16"), **pb("x", x),
           x_bf16=int(form[1] == "bf16"), **pb("gamma", g), **pb("dx_accum", acc), **pb("dx_bf16", dxb), **pb("dgamma", dg), **pb("dbeta", db),
           **pb("colsum", cs), **pb("scratch", sc), rows=rows, d=d)
    return dict(acc=acc.cpu(), dxb=dxb.cpu(), dgamma=dg.cpu() if dg else None, dbeta=db.cpu() if db else None, colsum=cs.cpu() if cs else None)


@pytest.mark.parametrize("form", T.LN_FORMS, ids=lambda f: f"dy_{f[0]}-x_{f[1]}")
@pytest.mark.parametrize("shape", T.LN_STREAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ln_stream_every_form_elementwise(lib, shape, form):
    rows, d = shape
    case = f"ln_stream_{rows}x{d}_{form[0]}_{form[1]}"
    c = T.ln_case(rows, d, 17 + rows + d, form)
    first = None
    for gamma, dests, colsum in ((True, True, True), (True, True, True), (False, True, False), (True, False, True)):
        got = ln_stream_launch(c, form, gamma, dests, colsum)
        r = T.ln_bwd_ref(c["x"], c["dy"], c["gamma"] if gamma else None, c["acc0"])
        tag = f"g{int(gamma)}d{int(dests)}c{int(colsum)}"
        report(case, "dx_accum_" + tag, worst_ratio(got["acc"], r["acc"], r["e_acc"]))
        assert same_bits(got["dxb"], T.bf(got["acc"])), (case, tag, "dx_bf16 is not the bf16 rounding of the dx_accum written")
        if dests:
            report(case, "dgamma_" + tag, worst_ratio(got["dgamma"], r["dgamma"][0], r["e_dgamma"][0]))
            report(case, "dbeta_" + tag, worst_ratio(got["dbeta"], r["dbeta"][0], r["e_dbeta"][0]))
        if colsum:
            s, es = T.colsum_ref(got["acc"].double())
            report(case, "colsum_" + tag, worst_ratio(got["colsum"], s, es))
        if first is None:
            first = got
        elif (gamma, dests, colsum) == (True, True, True):
            assert all(same_bits(first[k], got[k]) for k in first), (case, "two launches differ")
        elif gamma:                                                             # null dgamma / dbeta change nothing else
            assert same_bits(first["acc"], got["acc"]) and same_bits(first["colsum"], got["colsum"])


@pytest.mark.parametrize("shape", T.LN_GROUP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_ln_group_form_elementwise(lib, shape):
    rpg, groups, d = shape
    M, case = rpg * groups, f"ln_group_{rpg}x{groups}x{d}"
    c = T.ln_case(M, d, 23 + rpg + d)
    segs = [(g * rpg, (g + 1) * rpg) for g in range(groups)]
    r = T.ln_bwd_ref(c["x"], c["dy"], c["gamma"], c["acc0"], segs)
    nbytes = T.ln_scratch_bytes(rpg, groups, d)
    assert lib.ditto_layernorm_bwd_scratch_bytes(rpg, groups, d) == nbytes
    runs = []
    for _ in range(2):
        dy, x, g = In(c["dy"]), In(c["x"]), In(c["gamma"])
        acc, dgb, sc = Out((M, d), F32, init=c["acc0"]), Out((groups, 2 * d), F32), scratch(nbytes)
        launch("ditto_layernorm_bwd", [dy, x, g], [acc, dgb, sc], dy=dy.p, x=x.p, gamma=g.p, dx_accum=acc.p, dgamma_dbeta=dgb.p, scratch=sc.p,
               scratch_bytes=sc.nbytes, rows_per_group=rpg, groups=groups, d=d)
        runs.append((acc.cpu(), dgb.cpu()))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    acc, dgb = runs[0]
    report(case, "dx_accum", worst_ratio(acc, r["acc"], r["e_acc"]))
    report(case, "dgamma", worst_ratio(dgb[:, :d], r["dgamma"], r["e_dgamma"]))
    report(case, "dbeta", worst_ratio(dgb[:, d:], r["dbeta"], r["e_dbeta"]))


@pytest.mark.parametrize("d", T.ADALN_D)
@pytest.mark.parametrize("lens", T.ADALN_LENS, ids=lambda l: "-".join(map(str, l)))
def test_adaln_packed_per_utterance(lib, lens, d):
    c = T.adaln_case(lens, d, 41 + d + lens[0])
    want, e = T.adaln_packed_ref(c)
    B, S, mx = len(lens), sum(lens), max(lens)
    nbytes = hip.call("ditto_bwd_adaln_packed_scratch_bytes", max_len=mx, B=B, d=d)
    assert nbytes == T.adaln_scratch_bytes(mx, B, d)
    runs = []
    for _ in range(2):
        dy, x, cu = In(c["dy"]), In(c["x"]), In(torch.tensor(c["cu"], dtype=torch.int32))
        dmod, sc = Out((B, 2 * d), F32), scratch(nbytes)
        launch("ditto_bwd_adaln_packed", [dy, x, cu], [dmod, sc], **pb("dy", dy), **pb("x", x), **pb("cu", cu), **pb("dmod", dmod), **pb("scratch", sc),
               B=B, S=S, max_len=mx, d=d)
        runs.append(dmod.cpu())
    assert same_bits(*runs)
    report(f"adaln_packed_{'-'.join(map(str, lens))}_{d}", "dmod", worst_ratio(runs[0], want, e))


# =========================================================== gated-MLP derivative ===========================================================
def gated_launch(pre, dact, M, F, fused):
    i_pre, i_dact = In(pre), In(dact)
    dpre = Out((M, 2 * F), BF16)
    cs, sc = (Out(2 * F, F32), scratch(256 * 2 * F * 4)) if fused else (None, None)
    launch("ditto_bwd_gated", [i_pre, i_dact], [dpre, cs, sc], **pb("dact", i_dact), **pb("pre", i_pre), **pb("dpre", dpre), **pb("colsum", cs),
           **pb("scratch", sc), M=M, F=F)
    return dpre.cpu(), cs.cpu() if cs else None


@pytest.mark.parametrize("M", T.GATED_M)
@pytest.mark.parametrize("F", T.GATED_F)
def test_gated_bwd_elementwise_with_and_without_bias_sums(lib, F, M):
    case = f"gated_{M}x{F}"
    c = T.gated_case(M, F, 51 + M + F)
    want, e, _ = T.gated_ref(c)
    pre = T.interleave(c["a"], c["g"])
    d_f, cs = gated_launch(pre, c["dy"], M, F, True)
    d_f2, cs2 = gated_launch(pre, c["dy"], M, F, True)
    d_u, _ = gated_launch(pre, c["dy"], M, F, False)
    assert same_bits(d_f, d_f2) and same_bits(cs, cs2), (case, "two launches differ")
    assert same_bits(d_f, d_u), (case, "the fused and the unfused form write different dpre")
    r = ((d_f.double() - want).abs() - torch.ldexp(torch.ones_like(want), torch.frexp(d_f.double())[1] - 9)).clamp_min(0) / e
    r = torch.where(torch.isfinite(d_f.double()), r, torch.full_like(r, math.inf)).view(M, F // 16, 2, 16)
    report(case, "da", float(r[:, :, 0].max()))
    report(case, "dg", float(r[:, :, 1].max()))
    s, es = T.colsum_ref(d_f.double())
    report(case, "bias_sums", worst_ratio(cs, s, es))


def test_gated_bwd_grid_stride_second_trip(lib):
    """(4104, 4096) without column sums crosses ew_grid's cap of 8192 workgroups: the fp64 bound on the first 8 and the last 16 rows, and
    the whole output bitwise against the same rows computed in launches of 512"""
    M, F = T.GATED_BIG
    assert M * F // 8 > 8192 * 256
    g = torch.Generator().manual_seed(5)
    a, gt = T.bf(2.5 * torch.randn(M, F, generator=g)), T.bf(4.0 * torch.randn(M, F, generator=g))
    dy = T.bf(torch.randn(M, F, generator=g) * torch.logspace(-2, 1.5, M)[torch.randperm(M, generator=g)][:, None])
    pre = T.interleave(a, gt)
    whole, _ = gated_launch(pre, dy, M, F, False)
    for lo, hi in ((0, 8), (M - 16, M)):
        want, e, _ = T.gated_ref(dict(a=a[lo:hi], g=gt[lo:hi], dy=dy[lo:hi]))
        report(f"gated_{M}x{F}", f"rows_{lo}_{hi}", worst_ratio(whole[lo:hi], want, e, stored_bf16=True))
    for lo in range(0, M, 512):
        hi = min(lo + 512, M)
        part, _ = gated_launch(pre[lo:hi], dy[lo:hi], hi - lo, F, False)
        assert same_bits(part, whole[lo:hi]), (lo, hi)


# =========================================================== column sums ===========================================================
def colsum_launch(x, M, n, ld, shift=0):
    xin = In(x.reshape(-1)[:(M - 1) * ld + n], shift)
    out = Out(n, F32)
    nbytes = hip.call("ditto_bwd_colsum_scratch_bytes", M=M, n=n)
    assert nbytes == T.colsum_scratch_bytes(M, n)
    sc = scratch(nbytes)
    launch("ditto_bwd_colsum", [xin], [out, sc], **pb("x", xin), x_bf16=int(x.dtype == BF16), **pb("out", out), **pb("scratch", sc), M=M, n=n, ld=ld)
    return out.cpu()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", T.COLSUM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_colsum_both_dtypes_strided(lib, case, dtype):
    M, n, ld = case
    x = T.scaled_rows(M, ld, 81 + M).to(dtype)
    x[:, n:] = NAN                                                               # the columns past n are never read
    s, e = T.colsum_ref(x[:, :n].double())
    a, b = colsum_launch(x, M, n, ld), colsum_launch(x, M, n, ld)
    assert same_bits(a, b)
    report(f"colsum_{M}x{n}x{ld}_{'bf16' if dtype == BF16 else 'f32'}", "out", worst_ratio(a, s, e))


def test_colsum_bf16_off_16_byte_alignment_takes_the_fallback(lib):
    M, n, ld = 33, 256, 768
    x = T.scaled_rows(M, ld, 81 + M).to(BF16)
    x[:, n:] = NAN
    s, e = T.colsum_ref(x[:, :n].double())
    got = colsum_launch(x, M, n, ld, shift=4)                                    # 8 bytes off
    report("colsum_33x256x768_bf16_shift8", "out", worst_ratio(got, s, e))
    xin = In(x.reshape(-1)[:(M - 1) * ld + n], 2)                                # 4 bytes off: refused, not launched
    out, sc = Out(n, F32), scratch(T.colsum_scratch_bytes(M, n))
    assert hip.call("ditto_bwd_colsum", **pb("x", xin), x_bf16=1, **pb("out", out), **pb("scratch", sc), M=M, n=n, ld=ld, stream=stream()) == hip.ERR_ARG


@pytest.mark.parametrize("case", T.REDUCE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reduce_partials_both_kernels(lib, case):
    chunks, n = case
    p = T.scaled_rows(chunks, n, 83 + chunks)
    s, e = T.colsum_ref(p.double())
    runs = []
    for _ in range(2):
        pin, out = In(p), Out(n, F32)
        launch("ditto_bwd_reduce_partials", [pin], [out], **pb("partial", pin), **pb("out", out), chunks=chunks, n=n)
        runs.append(out.cpu())
    assert same_bits(*runs)
    report(f"reduce_{chunks}x{n}", "out", worst_ratio(runs[0], s, e))


# =========================================================== transpose, packers ===========================================================
@pytest.mark.parametrize("cols", T.TRANSPOSE_COLS)
@pytest.mark.parametrize("rows", T.TRANSPOSE_ROWS)
def test_transpose_bf16_pads_with_zero(lib, rows, cols):
    ld = cols + 8
    src = T.bf(T.scaled_rows(rows, ld, 87 + rows + cols))
    src[:, cols:] = NAN
    for ldT in ((rows + 63) // 64 * 64, (rows + 63) // 64 * 64 + 64):
        sin = In(src.reshape(-1)[:(rows - 1) * ld + cols])
        dst = Out((cols, ldT), BF16)
        launch("ditto_bwd_transpose_bf16", [sin], [dst], **pb("src", sin), **pb("dst", dst), rows=rows, cols=cols, ld=ld, ldT=ldT, nz_o=1, nz_i=1,
               s_o=0, s_i=0, d_z=0)
        assert same_bits(dst.cpu(), T.transpose_ref(src, rows, cols, ldT)), (rows, cols, ldT)


def test_transpose_bf16_batched_head_slices(lib):
    rows, cols, nzo, nzi, ldT = 65, 72, 2, 3, 128                                # src [nzo, rows, nzi * cols]: s_i = cols, as attention slices heads
    ld, s_o, d_z = nzi * cols, rows * nzi * cols, cols * ldT + 64                # a gap between the slices of dst keeps the pattern
    src = T.bf(T.scaled_rows(nzo * rows, ld, 89)).view(nzo, rows, ld)
    sin, dst = In(src), Out((nzo * nzi - 1) * d_z + cols * ldT, BF16)
    launch("ditto_bwd_transpose_bf16", [sin], [dst], **pb("src", sin), **pb("dst", dst), rows=rows, cols=cols, ld=ld, ldT=ldT, nz_o=nzo, nz_i=nzi,
           s_o=s_o, s_i=cols, d_z=d_z)
    got, written = dst.cpu(), torch.zeros(dst.n, dtype=torch.bool)
    for z in range(nzo * nzi):
        want = T.transpose_ref(src[z // nzi][:, (z % nzi) * cols:], rows, cols, ldT)
        assert same_bits(got[z * d_z:z * d_z + cols * ldT].view(cols, ldT), want), z
        written[z * d_z:z * d_z + cols * ldT] = True
    assert dst.untouched(written)


@pytest.mark.parametrize("case", T.PACK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pack_and_unpack_follow_the_row_map(lib, case):
    rows, cols, blk, mult, off = case
    m = T.pack_map(rows, blk, mult, off)
    last, ldT = int(m[-1]), T.pack_ldT(rows, blk, mult, off)
    W = T.scaled_rows(rows, cols, 91 + off)
    src, dst = In(W), Out((cols - 1) * ldT + last + 1, BF16)
    launch("ditto_bwd_pack_bf16_t", [src], [dst], **pb("src", src), **pb("dst", dst), rows=rows, cols=cols, ldT=ldT, blk=blk, mult=mult, row_off=off)
    want = torch.zeros(cols, ldT, dtype=BF16)
    reached = torch.zeros(cols, ldT, dtype=torch.bool)
    want[:, m], reached[:, m] = T.bf(W).T, True
    n = dst.n
    assert same_bits(dst.cpu()[reached.reshape(-1)[:n]], want.reshape(-1)[:n][reached.reshape(-1)[:n]])
    assert dst.untouched(reached.reshape(-1)[:n])                                 # what the map never reaches keeps the pattern
    assert hip.call("ditto_bwd_pack_bf16_t", **pb("src", src), **pb("dst", dst), rows=rows, cols=cols, ldT=last, blk=blk, mult=mult, row_off=off,
                    stream=stream()) == hip.ERR_SHAPE                             # an ldT that does not cover the map is refused
    packed = T.scaled_rows(last + 1, cols, 93 + off)
    packed[~torch.isin(torch.arange(last + 1), m)] = NAN                          # the rows the map skips are never read
    pin, out = In(packed), Out((rows, cols), F32)
    kw = dict(**pb("src", pin), **pb("dst", out), rows=rows, cols=cols, blk=blk, mult=mult, row_off=off)
    if cols % 4:                                                                  # refused by design: 16-byte rows
        assert hip.call("ditto_bwd_unpack_rows", stream=stream(), **kw) == hip.ERR_SHAPE
    else:
        launch("ditto_bwd_unpack_rows", [pin], [out], **kw)
        assert same_bits(out.cpu(), packed[m])
    vin, vout = In(packed[:, 0].contiguous()), Out(rows, F32)
    launch("ditto_bwd_unpack_vec", [vin], [vout], **pb("src", vin), **pb("dst", vout), rows=rows, blk=blk, mult=mult, row_off=off)
    assert same_bits(vout.cpu(), packed[m, 0])


def test_unpack_rows_identity_map_at_a_served_width(lib):
    rows, cols, blk, mult, off = T.UNPACK_CASES[2]
    packed = T.scaled_rows(rows, cols, 95)
    pin, out = In(packed), Out((rows, cols), F32)
    launch("ditto_bwd_unpack_rows", [pin], [out], **pb("src", pin), **pb("dst", out), rows=rows, cols=cols, blk=blk, mult=mult, row_off=off)
    assert same_bits(out.cpu(), packed)


@pytest.mark.parametrize("d", [1, 300])
def test_embedding_scatter_add_clamps_and_accumulates_in_order(lib, d):
    V = 5
    c = T.scatter_case(V, d, 97 + d)
    runs = []
    for _ in range(2):
        dr, ids, tab = In(c["drows"]), In(c["ids"]), Out((V, d), F32, init=c["table0"])
        launch("ditto_bwd_embedding_scatter_add", [dr, ids], [tab], **pb("drows", dr), **pb("ids", ids), **pb("dtable", tab), B=6, V=V, d=d)
        runs.append(tab.cpu())
    assert same_bits(runs[0], T.scatter_ref(c, V)) and same_bits(*runs)


# =========================================================== dropout softmax rows ===========================================================
@pytest.mark.parametrize("p", T.SOFTMAX_P)
@pytest.mark.parametrize("rpb", T.SOFTMAX_RPB)
@pytest.mark.parametrize("Skv", T.SOFTMAX_SKV)
def test_softmax_rows_forward_and_backward(lib, Skv, rpb, p):
    c = T.softmax_case(rpb, Skv, 61 + Skv + rpb)
    r = T.softmax_rows_ref(c, p)
    nrows, ld, case = c["nrows"], c["ld"], f"softmax_{rpb}x{Skv}_p{p}"
    assert nrows % 4 and T.SOFTMAX_BH0
    com = dict(nrows=nrows, rows_per_bh=rpb, Skv=Skv, ld=ld, scale=T.SOFTMAX_SCALE, seed=T.SOFTMAX_SEED, layer=T.SOFTMAX_LAYER, bh0=T.SOFTMAX_BH0, p_drop=p)
    ext = (nrows - 1) * ld + Skv
    runs = []
    for _ in range(2):
        S, dP = In(c["S"].reshape(-1)[:ext]), In(c["dP"].reshape(-1)[:ext])
        P, dS = Out((nrows, ld), BF16), Out((nrows, ld), BF16)
        launch("ditto_bwd_softmax_drop_rows", [S], [P], **pb("S", S), **pb("P", P), **com)
        launch("ditto_bwd_softmax_rows", [S, dP], [dS], **pb("S", S), **pb("dPd", dP), **pb("dS", dS), **com)
        runs.append((P.cpu(), dS.cpu()))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    P, dS = runs[0]
    assert torch.equal(P[:, :Skv] != 0, r["keep"] != 0), (case, "the forward's mask is not the oracle's")
    assert not bits(P[:, Skv:]).any() and not bits(dS[:, Skv:]).any(), (case, "padding columns are not +0")
    report(case, "P", worst_ratio(P, r["P"], r["e_P"], stored_bf16=True))
    report(case, "dS", worst_ratio(dS, r["dS"], r["e_dS"], stored_bf16=True))


# =========================================================== small linear ===========================================================
@pytest.mark.parametrize("silu", [1, 0], ids=["silu", "plain"])
@pytest.mark.parametrize("case", T.SMALL_LINEAR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_small_linear_three_modes(lib, case, silu):
    B, I, O = case
    c = T.small_linear_case(B, I, O, 71 + I)
    name, tag = "ditto_bwd_small_linear", f"small_linear_{B}x{I}x{O}_{'silu' if silu else 'plain'}"
    dims = dict(B=B, I=I, O=O, silu_in=silu)
    null = {"dy": None, "dy_bytes": 0}
    for bias in (True, False):
        x, W, b, dy = In(c["x"]), In(c["W"]), In(c["bias"]) if bias else None, In(c["dy"])
        y = Out((B, O), F32)
        launch(name, [x, W, b], [y], mode=hip.SMALL_LINEAR_FWD, **pb("x", x), **pb("W", W), **null, **pb("out", y), **pb("bias", b), **dims)
        want, e = T.small_linear_ref(c, 0, bool(silu), bias)
        report(tag, f"y_bias{int(bias)}", worst_ratio(y.cpu(), want, e))
        dW, db = Out((O, I), F32), Out(O, F32) if bias else None
        launch(name, [x, dy], [dW, db], mode=hip.SMALL_LINEAR_BWD_W, **pb("x", x), W=None, W_bytes=0, **pb("dy", dy), **pb("out", dW), **pb("bias", db), **dims)
        want, e, wb, eb = T.small_linear_ref(c, 1, bool(silu))
        report(tag, f"dW_bias{int(bias)}", worst_ratio(dW.cpu(), want, e))
        if bias:
            report(tag, "dbias", worst_ratio(db.cpu(), wb, eb))
    x, W, dy, dx = In(c["x"]), In(c["W"]), In(c["dy"]), Out((B, I), F32)
    launch(name, [x, W, dy], [dx], mode=hip.SMALL_LINEAR_BWD_X, **pb("x", x), **pb("W", W), **pb("dy", dy), **pb("out", dx), bias=None, bias_bytes=0, **dims)
    want, e = T.small_linear_ref(c, 2, bool(silu))
    report(tag, "dx", worst_ratio(dx.cpu(), want, e))
    dx2 = Out((B, I), F32)
    launch(name, [x, W, dy], [dx2], mode=hip.SMALL_LINEAR_BWD_X, **pb("x", x), **pb("W", W), **pb("dy", dy), **pb("out", dx2), bias=None, bias_bytes=0, **dims)
    assert same_bits(dx.cpu(), dx2.cpu())


# =========================================================== the valid call of every host-test argument set ===========================================================
def test_the_valid_call_of_every_host_argument_set_succeeds(lib):
    for label, (name, args, _) in T.host_arg_sets().items():
        boxes = []

        def address(b):
            boxes.append(Out(b.nbytes, torch.uint8, init=torch.zeros(b.nbytes, dtype=torch.uint8)))   # zeros: ids, offsets and values all in range
            assert boxes[-1].p % 16 == 0
            return boxes[-1].p
        kw = T.materialise(args, address)
        kw["stream"] = stream()
        rc = hip.call(name, **kw)
        assert rc == hip.OK, (label, rc, lib.ditto_last_error().decode())
        torch.cuda.synchronize()
        assert all(b.clean() for b in boxes), label
