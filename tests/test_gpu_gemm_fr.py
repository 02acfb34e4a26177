"""The full-row GEMM family at kernel level (csrc/gemm_frd.hip, csrc/gemm_fr64.hip, csrc/gemm_lnq.hip over csrc/fr_common.h) and the
stand-alone LayerNorm launches they claim to match, against the fp64 references and the derived elementwise bounds of gemm_fr_ref.py.
Every value assertion is elementwise (worst_ratio <= 1) or bitwise; -s prints one `FR_RATIO <case> <worst>` line per case.

Every operand lives inside a larger allocation with 4 rows above and 256 below (a tile is at most 128 rows: an unclamped access of a
ragged last tile lands in the band, not outside the allocation), at strides above the logical width: lda = K + 48 with A at column 16,
ldo = ldr = N + 24, ldu = N + 40 (fp8 u: N + 48 bytes), ldh = d + 12 (fp32) / d + 16 (bf16).  What the kernel must not read is NaN, what
it must not write is a (NaN) sentinel, and afterwards the bands are intact and the inputs bit-identical.  bias, gamma and beta are spread
over three decades in a shuffled order, the residual is a hash of (row, column), and the last four rows of every case are
gemm_fr_ref.special_rows (variance 0, variance 1e-6, mean 300, two half-row means).

Measured on an MI355X (2026-10-19), worst FR_RATIO per group: a (N = 768, fp32 stream) 0.114, b (N = 1024) 0.057 with u as bf16 and
0.046 as e4m3, c (bf16 stream) 0.008, d (exact integers: h is bitwise, the ratio is u's) 0.014, e (lnq) 0.237 through a general W and 0.003
through the identity, f (LayerNorm launches) 0.517 with gamma | beta (the fp32 output of ditto_layernorm_dual, which has no store grant)
and 0.039 without.  Groups b (fp8), c and d are below 0.05: the term that dominates their bounds is the one that is linear in the length of a sum whose order is not known a priori, (K + 2) 2^-24 (|A| |W|^T + |bias| + |residual|) for h and, for u,
the mean's (d + 1) 2^-24 mean|x| rstd and the propagated h bound: correct fp32 sums err like the square root of their length, so they
sit at a few percent of it, and the terms cannot be tightened without fixing the summation order inside and between the MFMAs, which
the kernels do not promise (the K-loop rotation changes it).  What keeps these groups sensitive all the same: h is pinned bit for bit
on the exact-integer data (every index map, every rotation), and every u, bf16 h and lnq output is a STORED value whose grant is half
an ulp of its own format, so a result one bf16 (or e4m3) ulp off leaves half an ulp over the grant: 2^-9 |u| against an arithmetic
bound of about 2^-15 |gamma t|: a ratio in the hundreds.  test_gemm_fr_ref.py shows it for each mutation a wrong kernel could be."""
import contextlib

import pytest
import torch

import gemm_fr_ref as R
from ditto_tts_amd import hip
from gpu_util import asym, stream
from test_gpu_gemm_fp8 import BELOW, TOP, _bits, _first_wrong, cached, guards_intact, window

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
OPTION_DEFAULTS = dict(fr_tile=0, fr_rot=1, fr_hb=0, fr_u_fp8=0, lnq_waves=8, lnq_ring=0)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return hip.lib()


@contextlib.contextmanager
def options(lib, **kw):
    try:
        for k, v in kw.items():
            hip.check(lib.ditto_set_option(k.encode(), v))
        yield
    finally:
        for k in kw:
            hip.check(lib.ditto_set_option(k.encode(), OPTION_DEFAULTS[k]))


def report(case, worst):
    print(f"FR_RATIO {case} {worst:.3f}")
    assert worst <= 1.0, (case, worst)


def ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------- guarded buffers -------------------------------------------------------------
def guarded_rows(x, ld, col0=0):
    """x [M, C] at column col0 of a NaN [TOP + M + BELOW, ld] buffer of x's type: (buffer, view of the valid rows from column col0)"""
    M, C = x.shape
    buf = torch.full((TOP + M + BELOW, ld), NAN, dtype=x.dtype, device=DEV)
    buf[TOP:TOP + M, col0:col0 + C] = x
    return buf, buf[TOP:, col0:]


def guarded_vec(v, pad=64):
    """fp32 vector with `pad` NaNs on either side (the view stays 16-byte aligned)"""
    if v is None:
        return None, None
    buf = torch.full((v.numel() + 2 * pad,), NAN, device=DEV)
    buf[pad:pad + v.numel()] = v
    return buf, buf[pad:]


def guarded_flat(x, pad=8192):
    buf = torch.full((x.numel() + 2 * pad,), NAN, dtype=x.dtype, device=DEV)
    buf[pad:pad + x.numel()] = x.reshape(-1)
    return buf, buf[pad:]


class Kept:
    def __init__(self, *bufs):
        self.keep = [(b, b.clone()) for b in bufs if b is not None]

    def intact(self):
        return all(torch.equal(_bits(b), _bits(c)) for b, c in self.keep)


# ------------------------------------------------------- ditto_gemm_ln_bf16: one launch -------------------------------------------------------
MODES = ["inplace", "separate", "nores", "nobias", "noln"]
MODES_ROTS = [(m, r) for m in MODES for r in (0, 3, 8) if (m, r) != ("inplace", 0)]      # (in place at rot 0: the every-shape tests)


def run_ln(lib, c, mode="inplace", tile=0, rot=0, hb=False, fp8=False):
    """one guarded, strided launch; returns (h [M, N] view, u [M, N] view or None) after the band and input checks"""
    M, K = c["A"].shape
    N = c["W"].shape[0]
    res, bias, ln = mode != "nores", mode != "nobias", mode != "noln"
    lda, ldo, ldu = K + 48, N + 24, N + (48 if fp8 else 40)
    Ab, Av = guarded_rows(c["A"], lda, 16)
    Wb, Wv = guarded_flat(R.pack_w(c["W"]))
    bb, bv = guarded_vec(c["bias"] if bias else None)
    gb, gv = guarded_vec(c["gamma"] if ln else None)
    eb, ev = guarded_vec(c["beta"] if ln else None)
    hkind = "bf16" if hb else "f32"
    hbuf, hview = window(M, ldo, hkind)
    r = c["res"].to(torch.bfloat16) if hb else c["res"]
    rb = rv = None
    if res and mode == "separate":
        rb, rv = guarded_rows(r, ldo)
    elif res:
        hview[TOP:TOP + M, :N] = r
        rv = hview[TOP:]
    ubuf = uview = None
    if ln:
        ubuf, uview = window(M, ldu, "u8" if fp8 else "bf16")
    kept = Kept(Ab, Wb, bb, gb, eb, rb)
    with options(lib, fr_tile=tile, fr_rot=rot, fr_hb=int(hb), fr_u_fp8=int(fp8)):
        hip.check(lib.ditto_gemm_ln_bf16(ptr(Av), lda, ptr(Wv), ptr(bv), ptr(rv), ptr(hview[TOP:]), ldo, ptr(gv), ptr(ev),
                                         ptr(uview[TOP:]) if ln else None, ldu, M, N, K, stream()))
        torch.cuda.synchronize()
    assert guards_intact(hbuf, M, 0, N, hkind) and kept.intact()
    if ln:
        assert guards_intact(ubuf, M, 0, N, "u8" if fp8 else "bf16")
    return hview[TOP:TOP + M, :N], uview[TOP:TOP + M, :N] if ln else None


def on_dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


def ln_case(M, N, K, stream_kind="f32", gscale=1.0):
    return cached(("fr", M, N, K, stream_kind, gscale), lambda: on_dev(R.case(M, N, K, 7 + M + K, stream_kind, gscale)))


def h_want(c, key, mode):
    def make():
        return R.h_ref(c["A"], c["W"], c["bias"] if mode != "nobias" else None, c["res"] if mode != "nores" else None)
    return cached(("h",) + key + (mode in ("nobias", "nores") and mode,), make)


def check_f32(case, c, key, mode, h, u, fp8=False):
    """h against fp64 from the operands; u against the fp64 LayerNorm of the h the kernel stored"""
    h64, hbnd = h_want(c, key, mode)
    worst = R.worst_ratio(h, h64, hbnd)
    if u is not None:
        want, e = R.layernorm(h, c["gamma"], c["beta"])
        if fp8:
            sat, sub = R.e4m3_edges(want)
            assert sat >= 32 and sub >= 32, (sat, sub)              # both edges of e4m3 are in the reference
            worst = max(worst, R.worst_ratio(R.deq(u.contiguous()), want, e, stored="e4m3"))
        else:
            worst = max(worst, R.worst_ratio(u, want, e, stored="bf16"))
    report(case, worst)


# ------------------------------------------------------- a. N = 768, fp32 stream -------------------------------------------------------
def run_768(lib, name, M, K, mode, rot):
    key = (M, 768, K, "f32", 1.0)
    c = ln_case(*key)
    outs = {}
    for tile in ((130, 64) if M >= 128 else (64,)):
        h, u = run_ln(lib, c, mode, tile=tile, rot=rot)
        check_f32(f"{name}/tile{tile}/M{M}K{K}/{mode}/rot{rot}", c, key, mode, h, u)
        outs[tile] = h
    if 130 in outs:
        assert torch.equal(_bits(outs[130].contiguous()), _bits(outs[64].contiguous())), _first_wrong(outs[130], outs[64])


@pytest.mark.parametrize("K", [64, 128, 192, 768, 3072])
@pytest.mark.parametrize("M", [64, 65, 127, 128, 129, 300, 1024, 1061])
def test_a_fp32_stream_768_every_shape(lib, M, K):
    """64 .. 127 rows run the 64-row twin alone; 1024 rows are 8 / 16 tiles and take fr_xcd_tile's remap, 1061 do not; one to three
    slabs of 64 exercise the ring prologue and the tail stages"""
    run_768(lib, "a", M, K, "inplace", 0)


@pytest.mark.parametrize("mode,rot", MODES_ROTS)
@pytest.mark.parametrize("K", [128, 768])
@pytest.mark.parametrize("M", [129, 1024, 1061])
def test_a_fp32_stream_768_modes_and_rotations(lib, M, K, mode, rot):
    run_768(lib, "a", M, K, mode, rot)


# ------------------------------------------------------- b. N = 1024 (gemm_fr64, NBW = 8) -------------------------------------------------------
def run_1024(lib, M, K, mode, rot, fp8=False):
    key = (M, 1024, K, "f32", 16.0 if fp8 else 1.0)
    c = ln_case(*key)
    h, u = run_ln(lib, c, mode, rot=rot, fp8=fp8)
    check_f32(f"b/{'fp8' if fp8 else 'bf16'}/M{M}K{K}/{mode}/rot{rot}", c, key, mode, h, u, fp8)


@pytest.mark.parametrize("K", [64, 256, 1024, 4096])
@pytest.mark.parametrize("M", [64, 65, 300, 512, 1061])
def test_b_fp32_stream_1024_every_shape(lib, M, K):
    run_1024(lib, M, K, "inplace", 0)


@pytest.mark.parametrize("mode,rot", MODES_ROTS)
@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("M", [65, 512, 1061])
def test_b_fp32_stream_1024_modes_and_rotations(lib, M, K, mode, rot):
    run_1024(lib, M, K, mode, rot)


@pytest.mark.parametrize("mode,rot", [("inplace", 0), ("separate", 3), ("nores", 8)])
@pytest.mark.parametrize("K", [64, 1024])
@pytest.mark.parametrize("M", [64, 300, 1061])
def test_b_fp8_layernorm_output(lib, M, K, mode, rot):
    """u as e4m3 bytes at a byte stride of N + 48; gamma scaled 16 so that the reference has outputs beyond +-448 and in the subnormal
    range (counted)"""
    run_1024(lib, M, K, mode, rot, fp8=True)


# ------------------------------------------------------- c. the bf16 stream (fr_hb, gemm_frd) -------------------------------------------------------
def check_hb(case, c, key, h, u):
    h64, hbnd = h_want(c, key, "inplace")
    worst = R.worst_ratio(h, h64, hbnd, stored="bf16")
    want, e = R.layernorm_of_perturbed(h64, hbnd, c["gamma"], c["beta"])
    report(case, max(worst, R.worst_ratio(u, want, e, stored="bf16")))


@pytest.mark.parametrize("rot", [0, 3])
@pytest.mark.parametrize("mode", ["inplace", "separate"])
@pytest.mark.parametrize("K", [64, 768, 3072])
@pytest.mark.parametrize("M", [128, 129, 255, 1024, 1061])
def test_c_bf16_stream(lib, M, K, mode, rot):
    """h = bf16 of the fp32 row (half a bf16 ulp on top of the accumulation bound); u = LayerNorm of the UNROUNDED row, against the
    LayerNorm of h64 within the propagated bound"""
    key = (M, 768, K, "bf16", 1.0)
    c = ln_case(*key)
    h, u = run_ln(lib, c, mode, tile=130, rot=rot, hb=True)
    check_hb(f"c/M{M}K{K}/{mode}/rot{rot}", c, key, h, u)


# ------------------------------------------------------- d. exact integers, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("rot", [0, 3, 8])
@pytest.mark.parametrize("K", [64, 192, 768])
@pytest.mark.parametrize("M", [129, 1024])
def test_d_exact_integers_bit_for_bit(lib, M, K, rot):
    """every partial sum is exact in fp32, so the fp32 h IS the fp64 h in any summation order: every index map of a, b and c,
    independently of any bound.  u is left to the bound (gemm_fr_ref.py: no row makes rstd a power of two)."""
    for N in (768, 1024):
        def make():
            c = R.exact_operands(M, N, K, 61)
            _, c["gamma"], c["beta"] = R.affine(N, 62)
            c = on_dev(c)
            h64, _ = R.h_ref(c["A"], c["W"], c["bias"], c["res"])
            assert torch.equal(h64.float().double(), h64)
            return c, h64
        c, h64 = cached(("exact", M, N, K), make)
        for mode in ("inplace", "separate"):
            for tile in ((130, 64) if N == 768 else (0,)):
                h, u = run_ln(lib, c, mode, tile=tile, rot=rot)
                assert torch.equal(h, h64.float()), (N, mode, tile, _first_wrong(h, h64.float()))
                want, e = R.layernorm(h, c["gamma"], c["beta"])
                report(f"d/N{N}/tile{tile}/M{M}K{K}/{mode}/rot{rot}", R.worst_ratio(u, want, e, stored="bf16"))
            if N == 768:
                h, u = run_ln(lib, c, mode, tile=130, rot=rot, hb=True)
                assert torch.equal(h, h64.float().to(torch.bfloat16)), (mode, _first_wrong(h, h64.float().to(torch.bfloat16)))
                want, e = R.layernorm(h64, c["gamma"], c["beta"])          # the unrounded row is exactly h64: nothing to propagate
                report(f"d/hb/M{M}K{K}/{mode}/rot{rot}", R.worst_ratio(u, want, e, stored="bf16"))


# ------------------------------------------------------- e. ditto_gemm_lnq_bf16 -------------------------------------------------------
def run_lnq(lib, x, g, b, W, bias, shape, h_bf16, opts):
    """one guarded, strided launch: rows at ldh = d + 12 (fp32) / d + 16 (bf16), out at ldo = d + 24"""
    M, d = x.shape
    ldh, ldo = d + (16 if h_bf16 else 12), d + 24
    xb, xv = guarded_rows(x.to(torch.bfloat16) if h_bf16 else x, ldh)
    gb, gv = guarded_vec(g)
    eb, ev = guarded_vec(b)
    bb, bv = guarded_vec(bias)
    Wb, Wv = guarded_flat(W)
    scratch = torch.empty(d * d * 2, dtype=torch.uint8, device=DEV)
    obuf, oview = window(M, ldo, "bf16")
    kept = Kept(xb, gb, eb, bb, Wb)
    with options(lib, **opts):
        hip.check(lib.ditto_gemm_lnq_bf16(ptr(xv), ldh, int(h_bf16), ptr(gv), ptr(ev), ptr(Wv), ptr(bv), ptr(oview[TOP:]), ldo, M, d, shape,
                                          ptr(scratch), stream()))
        torch.cuda.synchronize()
    assert guards_intact(obuf, M, 0, d, "bf16") and kept.intact()
    return oview[TOP:TOP + M, :d]


def lnq_case(M, d, h_bf16):
    def make():
        x = R.lnq_rows(M, d, 21 + M, h_bf16).to(DEV)
        bias, g, b = (t.to(DEV) for t in R.affine(d, 22))
        W = (asym((d, d), 23) / d ** 0.5).to(torch.bfloat16).to(DEV)
        return x, g, b, W, bias, R.lnq_ref(x, g, b, W, bias), R.lnq_ref(x, g, b, W, None), R.layernorm(x, g, b)
    return cached(("lnq", M, d, h_bf16), make)


def check_lnq(lib, name, M, d, shape, h_bf16, opts):
    x, g, b, W, bias, with_bias, no_bias, (y64, e_ln) = lnq_case(M, d, h_bf16)
    worst = 0.0
    for bv, (want, e) in ((bias, with_bias), (None, no_bias)):
        worst = max(worst, R.worst_ratio(run_lnq(lib, x, g, b, W, bv, shape, h_bf16, opts), want, e, stored="bf16"))
    report(f"e/{name}/M{M}", worst)
    # identity W: out IS the bf16 rounding of the kernel's normalised row: against the fp64 LayerNorm within the LayerNorm bound
    eye = torch.eye(d, dtype=torch.bfloat16, device=DEV)
    report(f"e/{name}/M{M}/identity", R.worst_ratio(run_lnq(lib, x, g, b, eye, None, shape, h_bf16, opts), y64, e_ln, stored="bf16"))


LNQ_VARIANTS = [dict(lnq_waves=8, lnq_ring=0, fr_rot=1), dict(lnq_waves=4, lnq_ring=0, fr_rot=5), dict(lnq_waves=4, lnq_ring=-1, fr_rot=16),
                dict(lnq_waves=8, lnq_ring=0, fr_rot=16)]


@pytest.mark.parametrize("variant", range(len(LNQ_VARIANTS)))
@pytest.mark.parametrize("shape", [32, 16])
@pytest.mark.parametrize("h_bf16", [False, True])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 200, 1024, 1061])
def test_e_lnq_768(lib, M, h_bf16, shape, variant):
    opts = dict(LNQ_VARIANTS[variant])
    if opts["lnq_ring"] < 0:
        opts["lnq_ring"] = 8 if shape == 32 else 4                      # the deep ring of the shape
    name = f"d768/shape{shape}/{'bf16' if h_bf16 else 'f32'}/waves{opts['lnq_waves']}ring{opts['lnq_ring']}rot{opts['fr_rot']}"
    check_lnq(lib, name, M, 768, shape, h_bf16, opts)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("M", [64, 100, 1061])
def test_e_lnq_1024(lib, M, variant):
    opts = dict(LNQ_VARIANTS[variant])
    check_lnq(lib, f"d1024/waves{opts['lnq_waves']}rot{opts['fr_rot']}", M, 1024, 32, False, opts)


# ------------------------------------------------------- f. the stand-alone LayerNorm launches -------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("d", [64, 256, 320, 768, 1024, 1472, 2048])
def test_f_layernorm_launches_elementwise(lib, d, affine):
    """ditto_layernorm_bf16 and ditto_layernorm_dual (fp32 and bf16 outputs): one to eight float4 chunks per lane, M in {1, 5, 70} plus
    the four special rows; rows after the last one of the sentinel-filled outputs stay intact"""
    worst = 0.0
    _, g, b = (t.to(DEV) for t in R.affine(d, 72))
    if not affine:
        g = b = None
    for M in (1, 5, 70):
        rows = M + R.N_SPECIAL
        x = R.lnq_rows(rows, d, 71 + M).to(DEV)
        keep = x.clone()
        want, e = R.layernorm(x, g, b)
        o1buf, o1 = window(rows, d, "bf16")
        hip.check(lib.ditto_layernorm_bf16(ptr(x), ptr(g), ptr(b), ptr(o1[TOP:]), rows, d, stream()))
        o2buf, o2 = window(rows, d, "bf16")
        f2buf, f2 = window(rows, d, "f32")
        hip.check(lib.ditto_layernorm_dual(ptr(x), ptr(g), ptr(b), ptr(f2[TOP:]), ptr(o2[TOP:]), rows, d, stream()))
        torch.cuda.synchronize()
        assert torch.equal(x, keep)
        for buf, kind in ((o1buf, "bf16"), (o2buf, "bf16"), (f2buf, "f32")):
            assert guards_intact(buf, rows, 0, d, kind)
        y1, y2, yf = o1[TOP:TOP + rows], o2[TOP:TOP + rows], f2[TOP:TOP + rows]
        assert torch.equal(y2, yf.to(torch.bfloat16))                   # the bf16 copy: the fp32 result, rounded
        worst = max(worst, R.worst_ratio(y1, want, e, stored="bf16"), R.worst_ratio(yf, want, e), R.worst_ratio(y2, want, e, stored="bf16"))
    report(f"f/d{d}/{'affine' if affine else 'plain'}", worst)


# ------------------------------------------------------- g. refusals -------------------------------------------------------
def test_g_gemm_ln_refusals_are_error_codes_not_launches(lib):
    M, K = 129, 128
    S, A = hip.ERR_SHAPE, hip.ERR_ARG
    for N in (768, 1024):
        c = on_dev(R.exact_operands(M, N, K, 91))
        _, g, b = (t.to(DEV) for t in R.affine(N, 92))
        Ab = torch.zeros(M + 8, K + 48, dtype=torch.bfloat16, device=DEV)
        Wp = R.pack_w(c["W"])
        out = torch.full((M + 8, N + 24), 1.0, device=DEV)             # rows at the ldo = ldr, ldu of `ok`
        res = torch.zeros(M + 8, N + 24, device=DEV)
        u = torch.full((M + 8, N + 40), 1.0, dtype=torch.bfloat16, device=DEV)
        names = ["A", "lda", "W", "bias", "residual", "out", "ldo", "gamma", "beta", "u", "ldu", "M", "N", "K"]
        ok = dict(A=Ab.data_ptr(), lda=K + 48, W=Wp.data_ptr(), bias=c["bias"].data_ptr(), residual=res.data_ptr(), out=out.data_ptr(),
                  ldo=N + 24, gamma=g.data_ptr(), beta=b.data_ptr(), u=u.data_ptr(), ldu=N + 40, M=M, N=N, K=K)

        def call(**change):
            a = {**ok, **change}
            return lib.ditto_gemm_ln_bf16(*[a[n] for n in names], stream())

        cases = [
            ({}, dict(N=512, ldo=1024, ldu=1024), S), ({}, dict(N=896, ldo=1024 + 24, ldu=1024 + 40), S), ({}, dict(M=63), S), ({}, dict(M=0), S),
            ({}, dict(K=96), S), ({}, dict(K=32), S), ({}, dict(K=0), S),
            ({}, dict(lda=K + 4), S), ({}, dict(lda=K - 8), S),
            ({}, dict(ldo=N - 4), S), ({}, dict(ldo=N + 2), S), ({}, dict(ldu=N - 8), S), ({}, dict(ldu=N + 4), S),
            ({}, dict(gamma=None), A), ({}, dict(beta=None), A), ({}, dict(u=None), A), ({}, dict(gamma=None, beta=None), A),
            ({}, dict(A=None), A), ({}, dict(W=None), A), ({}, dict(out=None), A),
        ] + [({}, {k: ok[k] + off}, A) for k in ("A", "out", "residual", "u", "bias", "gamma", "beta", "W") for off in (4, 8)]
        if N == 768:
            cases += [(dict(fr_hb=1, fr_tile=130), dict(ldo=N + 4), S), (dict(fr_hb=1, fr_tile=130), dict(ldo=N - 8), S),
                      (dict(fr_u_fp8=1), {}, S), (dict(fr_hb=1, fr_u_fp8=1), {}, S)]
        else:
            cases += [(dict(fr_u_fp8=1), dict(ldu=N + 8), S), (dict(fr_u_fp8=1), dict(ldu=N - 16), S),
                      (dict(fr_u_fp8=1), dict(gamma=None, beta=None, u=None), S), (dict(fr_hb=1), {}, S)]
        for opts, change, code in cases:
            with options(lib, **opts):
                got = call(**change)
            assert got == code, (N, opts, change, got)
        if N == 768:            # the bf16 stream exists on the 128-row kernel alone: a launch the 64-row kernel would take is an error
            with options(lib, fr_hb=1, fr_tile=64):
                assert call() != hip.OK
        torch.cuda.synchronize()
        assert bool((out == 1.0).all()) and bool((u == 1.0).all())
        assert call() == hip.OK                                         # and the unchanged arguments do launch
        torch.cuda.synchronize()
        assert not bool((out[:M, :N] == 1.0).all()) and bool((out[:M, N:] == 1.0).all()) and bool((out[M:] == 1.0).all())


def test_g_gemm_lnq_refusals_are_error_codes_not_launches(lib):
    M, d = 70, 768
    S, A = hip.ERR_SHAPE, hip.ERR_ARG
    xb = torch.zeros(M + 8, d + 12, device=DEV)                         # rows at the ldh, ldo of `ok`
    bias, g, b = (t.to(DEV) for t in R.affine(d, 94))
    W = torch.eye(d, dtype=torch.bfloat16, device=DEV)
    scratch = torch.empty(d * d * 2 + 256, dtype=torch.uint8, device=DEV)
    out = torch.full((M + 8, d + 24), 1.0, dtype=torch.bfloat16, device=DEV)
    names = ["h", "ldh", "h_is_bf16", "gamma", "beta", "W", "bias", "out", "ldo", "M", "d", "shape", "scratch"]
    ok = dict(h=xb.data_ptr(), ldh=d + 12, h_is_bf16=0, gamma=g.data_ptr(), beta=b.data_ptr(), W=W.data_ptr(), bias=bias.data_ptr(),
              out=out.data_ptr(), ldo=d + 24, M=M, d=d, shape=32, scratch=scratch.data_ptr())

    def call(**change):
        a = {**ok, **change}
        return lib.ditto_gemm_lnq_bf16(*[a[n] for n in names], stream())

    cases = [
        (dict(d=512), S), (dict(d=1024, shape=16, ldh=1024 + 12, ldo=1024 + 24), S), (dict(d=1024, h_is_bf16=1, ldh=1024 + 16, ldo=1024 + 24), S),
        (dict(M=0), A), (dict(ldh=d - 4), A), (dict(ldh=d + 2), A), (dict(ldo=d - 8), A), (dict(ldo=d + 4), A), (dict(shape=8), A),
        (dict(h=None), A), (dict(gamma=None), A), (dict(beta=None), A), (dict(W=None), A), (dict(out=None), A), (dict(scratch=None), A),
        (dict(scratch=ok["scratch"] + 128), A),
        (dict(h=ok["h"] + 4), A), (dict(h=ok["h"] + 8), A), (dict(h=ok["h"] + 4, h_is_bf16=1, ldh=d + 16), A),
    ] + [({k: ok[k] + off}, A) for k in ("out", "gamma", "beta", "bias") for off in (4, 8)]
    for change, code in cases:
        assert call(**change) == code, (change, call(**change))
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())
    assert call(h=ok["h"] + 8, h_is_bf16=1, ldh=d + 16) == hip.OK        # bf16 rows: 8-byte loads
    assert call() == hip.OK
    torch.cuda.synchronize()
    assert not bool((out[:M, :d] == 1.0).all()) and bool((out[:M, d:] == 1.0).all()) and bool((out[M:] == 1.0).all())
