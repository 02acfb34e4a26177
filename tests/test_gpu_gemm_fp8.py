"""The fp8 GEMM family at kernel level (csrc/gemm256.hip gemm256_kernel<EPI, true, true, FLAT>: every epilogue the model launches,
every stride, every edge) and the two fp8 row kernels, against the fp64 references and the derived elementwise bounds of
gemm_fp8_ref.py.  Every value assertion is elementwise (worst_ratio <= 1) or bitwise; -s prints one `FP8_RATIO <case> <worst>` line
per case.  The launches go through ditto_gemm_epilogue_fp8, which fills a launch as the model does (ldw, w_rows, ldr != ldo,
out2_bf16, the QKV + RoPE epilogue).

Every operand lives inside a larger allocation with 256 slack rows (a tile is 256 rows: an unclamped access of a ragged last tile
lands in the band, not outside the allocation); what the kernel must not read is NaN (byte 0x7F for fp8), what it must not write is
a sentinel, and afterwards the bands are intact and the inputs bit-identical.  The weight rows (and with them the per-column scales)
and the bias are spread over three decades in a shuffled order, so a scale or a bias from the wrong column or the wrong tile moves
the result by orders of magnitude, not by a few percent.

Each case runs under three gemm_flags: 321 (straight-line epilogue, flat K loop at even K-tile counts), 321 + 1024 (general epilogue,
scales read from global memory), 321 + 16384 (prologue between K loop and epilogue).

Measured on an MI355X (2026-10-19), worst FP8_RATIO per group: a (plain epilogues) 0.216, b (tile switch) 0.094, c is bitwise,
d (QKV + RoPE) 0.613 table-free / 0.056 from tables, e (gated, fp8 output) 0.045, LayerNorm 0.002, quantiser 1.000 (elements next
to an e4m3 tie: the bound is half an ulp plus three fp32 roundings).  The accumulation term is the MEASURED one of gemm_fp8_ref.py:
against the derived (K + 2) 2^-24 term the same correct launches reached 1.52 at K = 128."""
import contextlib
import ctypes as C

import pytest
import torch

import gemm_epi_ref as E
import gemm_fp8_ref as R
from ditto_tts_amd import hip
from gpu_util import asym, stream
from test_gpu_gemm_epilogues import BF_SENT, F32_SENT

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8_SENT = 0x5A                    # a finite e4m3 byte (13.0)
NAN8 = 0x7F
FLAGS = [321, 321 + 1024, 321 + 16384]
TOP, BELOW = 4, 256


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return hip.lib()


@contextlib.contextmanager
def forced(lib, flags):
    hip.check(lib.ditto_set_option(b"gemm_flags", flags))
    try:
        yield
    finally:
        hip.check(lib.ditto_set_option(b"gemm_flags", 321))


def launch(lib, epi, wscale, rc_only=False, **kw):
    a = hip.GemmEpilogueArgs()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    st = C.c_int(-1)
    rc = lib.ditto_gemm_epilogue_fp8(C.byref(a), None if wscale is None else wscale.data_ptr(), epi, C.byref(st), stream())
    if rc_only:
        return rc, st.value
    hip.check(rc)
    assert st.value == 256, st.value
    return st.value


def quant(lib):
    def q(w):
        rows, cols = w.shape
        out = torch.empty(rows, cols, dtype=torch.uint8, device=DEV)
        sc = torch.empty(rows, dtype=torch.float32, device=DEV)
        hip.check(lib.ditto_quantize_rows_fp8(w.data_ptr(), rows, cols, out.data_ptr(), sc.data_ptr(), stream()))
        return out, sc
    return q


_cache = {}


def cached(key, fn):
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        _cache[key] = fn()
    return _cache[key]


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def report(case, worst):
    print(f"FP8_RATIO {case} {worst:.3f}")
    assert worst <= 1.0, (case, worst)


# ------------------------------------------------------------- guarded buffers -------------------------------------------------------------
def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Inputs:
    """A at column offset 16 of a [TOP + M + 256, K + 48] byte buffer, W in [N + 256, K + 32], bias / wscale with 64 elements of
    slack: NaN wherever the kernel must not read (W rows >= w_rows included)"""

    def __init__(self, Aq, Wq, ws, b, w_rows=0):
        M, K = Aq.shape
        N = Wq.shape[0]
        self.lda, self.ldw = K + 48, K + 32
        self.Ab = torch.full((TOP + M + BELOW, self.lda), NAN8, dtype=torch.uint8, device=DEV)
        self.Ab[TOP:TOP + M, 16:16 + K] = Aq
        wr = w_rows or N
        self.Wb = torch.full((N + BELOW, self.ldw), NAN8, dtype=torch.uint8, device=DEV)
        self.Wb[:wr, :K] = Wq[:wr]
        self.vecs = []
        for v in (b, ws):
            vb = None
            if v is not None:
                vb = torch.full((N + 64,), float("nan"), device=DEV)
                vb[:N] = v
            self.vecs.append(vb)
        self.bias, self.ws = self.vecs
        self.kw = dict(A=self.Ab.data_ptr() + TOP * self.lda + 16, lda=self.lda, W=self.Wb, ldw=self.ldw, w_rows=w_rows, M=M, N=N, K=K)
        if b is not None:
            self.kw["bias"] = self.bias
        self.keep = [(t, t.clone()) for t in (self.Ab, self.Wb, self.bias, self.ws) if t is not None]

    def intact(self):
        return all(torch.equal(_bits(t), _bits(c)) for t, c in self.keep)


_KIND = {"f32": (torch.int32, F32_SENT, torch.float32), "bf16": (torch.int16, BF_SENT, torch.bfloat16), "u8": (torch.uint8, U8_SENT, torch.uint8)}


def window(M, ld, kind):
    """[TOP + M + 256, ld] filled with the sentinel (as raw bits, and viewed as the output type)"""
    raw_t, s, t = _KIND[kind]
    buf = torch.full((TOP + M + BELOW, ld), s, dtype=raw_t, device=DEV)
    return buf, buf.view(t)


def guards_intact(buf, M, lo, hi, kind):
    """only rows TOP .. TOP + M, columns lo .. hi may have changed"""
    s = _KIND[kind][1]
    return bool((buf[:TOP] == s).all() and (buf[TOP + M:] == s).all() and (buf[TOP:TOP + M, hi:] == s).all() and
                (buf[TOP:TOP + M, :lo] == s).all())


# ---------------------------------------------------------------- the cases ----------------------------------------------------------------
def plain_case(lib, M, N, K, seed=31):
    def make():
        Aq, Wq, ws, b = R.operands(M, N, K, seed, DEV, quant(lib))
        want, accb = R.linear(Aq, Wq, ws, b)
        res = asym((min(M, 257), N), seed + 5).float().to(DEV)[torch.arange(M, device=DEV) % 257]   # (period 257: no multiple of a tile)
        return Aq, Wq, ws, b, want, accb, res
    return cached(("plain", M, N, K, seed), make)


def run_plain(lib, mode, Aq, Wq, ws, b, res, flags, w_rows=0):
    """one launch of epilogue 0 (`bf16`), 4 (`f32`) or 1 (`res_inplace`: residual == out; `res_side`: a separate residual at
    ldr != ldo and the bf16 side copy at column offset N of a [rows, 2 N] buffer); returns the valid output(s) after the band and
    input checks"""
    M, K = Aq.shape
    N = Wq.shape[0]
    inp = Inputs(Aq, Wq, ws, b, w_rows)
    kind = "bf16" if mode == "bf16" else "f32"
    ldo = N + 24
    buf, view = window(M, ldo, kind)
    kw = dict(inp.kw, out=view[TOP:], ldo=ldo)
    side = None
    if mode == "res_inplace":
        view[TOP:TOP + M, :N] = res
        kw.update(residual=view[TOP:], ldr=ldo)
    elif mode == "res_side":
        ldr = N + 12
        rb = torch.full((M + BELOW, ldr), float("nan"), device=DEV)
        rb[:M, :N] = res
        rkeep = rb.clone()
        b2, v2 = window(M, 2 * N, "bf16")
        kw.update(residual=rb, ldr=ldr, out2_bf16=v2[TOP:].data_ptr() + 2 * N, ldo2=2 * N)
    with forced(lib, flags):
        launch(lib, {"bf16": 0, "f32": 4}.get(mode, 1), inp.ws, **kw)
    torch.cuda.synchronize()
    assert guards_intact(buf, M, 0, N, kind) and inp.intact()
    if mode == "res_side":
        assert guards_intact(b2, M, N, 2 * N, "bf16") and torch.equal(_bits(rb), _bits(rkeep))
        side = v2[TOP:TOP + M, N:]
    return view[TOP:TOP + M, :N], side


def check_plain(case, mode, got, side, want, accb, res, cols):
    if mode == "bf16":
        r = R.worst_ratio(got[:, :cols], want[:, :cols], accb[:, :cols], stored="bf16")
    elif mode == "f32":
        r = R.worst_ratio(got[:, :cols], want[:, :cols], accb[:, :cols])
    else:
        wres = want + res.double()
        r = R.worst_ratio(got[:, :cols], wres[:, :cols], (accb + 2 * R.G * wres.abs())[:, :cols])
        if side is not None:
            assert torch.equal(side[:, :cols], got[:, :cols].to(torch.bfloat16))      # the side copy: the fp32 result, rounded
    report(case, r)


# ----------------------------------------------------------- a. plain epilogues 0, 1, 4 -----------------------------------------------------------
PLAIN_SHAPES = [(64, 16, 128), (300, 320, 128), (513, 2336, 384), (777, 1088, 256)]
MODES = ["bf16", "f32", "res_inplace", "res_side"]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,K", PLAIN_SHAPES)
def test_plain_epilogues(lib, M, N, K, mode, flags):
    Aq, Wq, ws, b, want, accb, res = plain_case(lib, M, N, K)
    got, side = run_plain(lib, mode, Aq, Wq, ws, b, res, flags)
    check_plain(f"a/{mode}/M{M}N{N}K{K}/flags{flags}", mode, got, side, want, accb, res, N)


@pytest.mark.parametrize("flags", FLAGS)
def test_null_wscale_is_bitwise_all_ones(lib, flags):
    M, N, K = 300, 320, 128
    Aq, Wq, _, b, _, _, res = plain_case(lib, M, N, K)
    want, accb = R.linear(Aq, Wq, None, b)
    none, _ = run_plain(lib, "f32", Aq, Wq, None, b, res, flags)
    ones, _ = run_plain(lib, "f32", Aq, Wq, torch.ones(N, device=DEV), b, res, flags)
    assert torch.equal(_bits(none.contiguous()), _bits(ones.contiguous()))
    report(f"a/null_wscale/M{M}N{N}K{K}/flags{flags}", R.worst_ratio(none, want, accb))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_w_rows_below_n(lib, mode, flags):
    """W rows >= w_rows = N - 16 are NaN bytes and never read: the columns below w_rows are right, the bands intact"""
    M, N, K = 513, 2336, 384
    Aq, Wq, ws, b, want, accb, res = plain_case(lib, M, N, K)
    got, _ = run_plain(lib, mode, Aq, Wq, ws, b, res, flags, w_rows=N - 16)
    check_plain(f"a/w_rows/{mode}/M{M}N{N}K{K}/flags{flags}", mode, got, None, want, accb, res, N - 16)


# ------------------------------------------------------------ b. the tile switch ------------------------------------------------------------
def switch_shape(n_tiles_n):
    """more tiles than CUs, so some workgroups take a second tile, with a ragged last row tile of 37 rows"""
    M = 256 * (n_cu() // n_tiles_n) + 37
    assert (M + 255) // 256 * n_tiles_n > n_cu()
    return M


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("mode", ["bf16", "f32", "res_inplace"])
@pytest.mark.parametrize("K", [256, 384])
def test_tile_switch_elementwise(lib, K, mode, flags):
    """five column tiles (the last 16 wide) whose scales and biases differ by decades: a workgroup's second tile read with the first
    tile's LDS slot is wrong by orders of magnitude.  K = 256 runs the flat K loop, K = 384 the prologue per tile."""
    N, M = 1040, switch_shape(5)
    Aq, Wq, ws, b, want, accb, res = plain_case(lib, M, N, K, seed=37)
    got, side = run_plain(lib, mode, Aq, Wq, ws, b, res, flags)
    check_plain(f"b/{mode}/M{M}N{N}K{K}/flags{flags}", mode, got, side, want, accb, res, N)


# ------------------------------------------------------- c. exact arithmetic, bit for bit -------------------------------------------------------
def exact_case(M, N, K):
    def make():
        Aq, Wq, ws, b = R.exact_operands(M, N, K, 61, DEV)
        want, _ = R.linear(Aq, Wq, ws, b)
        assert torch.equal(want.float().double(), want)
        res = torch.randint(-8, 9, (M, N), generator=torch.Generator().manual_seed(62)).float().to(DEV)
        return Aq, Wq, ws, b, want, res
    return cached(("exact", M, N, K), make)


def _first_wrong(got, want):
    bad = (got != want).nonzero()
    return f"first wrong (row, col): {bad[0].tolist()} of {bad.shape[0]}" if bad.numel() else ""


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", PLAIN_SHAPES + ["switch"])
def test_exact_integers_bit_for_bit(lib, shape, flags):
    """A in [-3, 3], W in [-2, 2], power-of-two scales with period 7, bias multiples of 2^-4: every partial sum is exact in fp32, so
    the fp32 output IS the fp64 reference whatever the order of the sums: every index map, independently of any bound"""
    M, N, K = (switch_shape(5), 1040, 256) if shape == "switch" else shape
    Aq, Wq, ws, b, want, res = exact_case(M, N, K)
    f32, _ = run_plain(lib, "f32", Aq, Wq, ws, b, res, flags)
    assert torch.equal(f32, want.float()), _first_wrong(f32, want.float())
    bf, _ = run_plain(lib, "bf16", Aq, Wq, ws, b, res, flags)
    assert torch.equal(bf, want.float().to(torch.bfloat16)), _first_wrong(bf, want.float().to(torch.bfloat16))
    for mode in ("res_inplace", "res_side"):
        r1, side = run_plain(lib, mode, Aq, Wq, ws, b, res, flags)
        assert torch.equal(r1, (want + res.double()).float()), (mode, _first_wrong(r1, (want + res.double()).float()))
        if side is not None:
            assert torch.equal(side, r1.to(torch.bfloat16))


# ------------------------------------------------------------- d. QKV + RoPE -------------------------------------------------------------
ROPE_SHAPES = [(256, 64, 63), (256, 200, 600), (384, 100, 300), (1024, 333, 999), (1024, 4096, 4396)]


def rope_tables(positions):
    invf = E.inv_freq().to(DEV)
    cs, sn = E.tables(invf, positions)
    return invf, E.freq_rev(invf).contiguous(), cs, sn


def rope_case(lib, d, rpb, M):
    def make():
        N, K, rc = 3 * d, d, 2 * d
        Aq, Wq, ws, b = R.operands(M, N, K, 51, DEV, quant(lib))
        pre, accb = R.linear(Aq, Wq, ws, b)
        invf, frev, cs, sn = rope_tables(max(M, rpb))          # tables cover every row index, not only every position
        pos = torch.arange(M, device=DEV) % rpb
        c64, s64 = E.rope_exact_tables(invf, pos)
        free = R.rope(pre, torch.arange(M, device=DEV), rc, c64, s64)
        bfree = R.rope_bound(pre, accb, rc, R.dtheta_table_free(pos, invf), E.E_SINCOS)
        tab, btab = R.rope(pre, pos, rc, cs, sn), R.rope_bound(pre, accb, rc)
        return Aq, Wq, ws, b, frev, cs, sn, free, bfree, tab, btab
    return cached(("rope", d, rpb, M), make)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("d,rpb,M", ROPE_SHAPES)
def test_qkv_rope(lib, d, rpb, M, flags):
    """the launch the fp8 model makes in every layer: table-free angles (the only form that takes the straight-line epilogue) and
    angles from tables; the v columns (>= rope_cols) are plain bias columns of the same reference"""
    N, K, rc = 3 * d, d, 2 * d
    Aq, Wq, ws, b, frev, cs, sn, free, bfree, tab, btab = rope_case(lib, d, rpb, M)
    ldo = N + 24
    for name, want, bound, extra in (("table-free", free, bfree, dict(rope_freq_rev=frev)), ("tables", tab, btab, {})):
        inp = Inputs(Aq, Wq, ws, b)
        buf, view = window(M, ldo, "bf16")
        with forced(lib, flags):
            launch(lib, 2, inp.ws, out=view[TOP:], ldo=ldo, rope_cos=cs, rope_sin=sn, rope_rows_per_batch=rpb, rope_cols=rc,
                   **inp.kw, **extra)
        torch.cuda.synchronize()
        assert guards_intact(buf, M, 0, N, "bf16") and inp.intact()
        report(f"d/{name}/d{d}rpb{rpb}M{M}/flags{flags}", R.worst_ratio(view[TOP:TOP + M, :N], want, bound, stored="bf16"))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("d", [256, 384])
def test_qkv_rope_pairing_and_sign_bit_for_bit(lib, d, flags):
    """Exact-integer data and no bias: acc is exact.  Tables with (cos, sin) = (0, 1) at odd positions and (1, 0) at even ones: the
    output is (-hi, lo) respectively (lo, hi), rounded to bf16, bit for bit."""
    rpb, M = 150, 450
    N, K, rc = 3 * d, d, 2 * d
    Aq, Wq, ws, _ = R.exact_operands(M, N, K, 63, DEV)
    acc, _ = R.linear(Aq, Wq, ws)
    odd = (torch.arange(max(M, rpb), device=DEV) % 2 == 1).float()[:, None].expand(-1, 32).contiguous()
    cs, sn = (1 - odd).contiguous(), odd
    pos = torch.arange(M, device=DEV) % rpb
    lo, hi = E._split(acc, rc)
    o = (pos % 2 == 1)[:, None, None]
    want = E._join(torch.where(o, -hi, lo), torch.where(o, lo, hi), acc[:, rc:]).float().to(torch.bfloat16)
    assert bool((lo != hi).float().mean() > 0.8)                # the partners differ: a wrong pairing shows
    inp = Inputs(Aq, Wq, ws, None)
    ldo = N + 24
    buf, view = window(M, ldo, "bf16")
    with forced(lib, flags):
        launch(lib, 2, inp.ws, out=view[TOP:], ldo=ldo, rope_cos=cs, rope_sin=sn, rope_rows_per_batch=rpb, rope_cols=rc, **inp.kw)
    torch.cuda.synchronize()
    assert guards_intact(buf, M, 0, N, "bf16") and inp.intact()
    got = view[TOP:TOP + M, :N]
    assert torch.equal(got, want), _first_wrong(got, want)


# ---------------------------------------------------------- e. gated MLP, fp8 output ----------------------------------------------------------
def gated_case(lib, M, N, K):
    def make():
        Aq, Wq, ws, b = R.operands(M, N, K, 41, DEV, quant(lib), gated_data=True)
        pre, accb = R.linear(Aq, Wq, ws, b)
        want, bound = R.gated(pre), R.gated_bound(pre, accb)
        sat, sub = R.e4m3_edges(want)
        assert sat >= 32 and sub >= 32, (sat, sub)              # both edges of e4m3 are in the reference
        return Aq, Wq, ws, b, want, bound
    return cached(("gated", M, N, K), make)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", [(300, 320, 128), (513, 2336, 384), (777, 1088, 256), "switch"])
def test_gated_fp8_output(lib, shape, flags):
    """W / bias rows interleaved [16 x fc1 | 16 x gate]: out e4m3 [M, N / 2] = gelu_erf(a) sigmoid(g), saturating, at a byte stride
    above N / 2.  `switch`: nine column tiles (the last 32 wide) and more tiles than CUs."""
    M, N, K = (switch_shape(9), 2080, 256) if shape == "switch" else shape
    Aq, Wq, ws, b, want, bound = gated_case(lib, M, N, K)
    inp = Inputs(Aq, Wq, ws, b)
    ldo = N // 2 + 24
    buf, view = window(M, ldo, "u8")
    with forced(lib, flags):
        launch(lib, 5, inp.ws, out=view[TOP:], ldo=ldo, **inp.kw)
    torch.cuda.synchronize()
    assert guards_intact(buf, M, 0, N // 2, "u8") and inp.intact()
    report(f"e/M{M}N{N}K{K}/flags{flags}", R.worst_ratio(R.deq(view[TOP:TOP + M, :N // 2].contiguous()), want, bound, stored="e4m3"))


# ------------------------------------------------------------ f. refusals ------------------------------------------------------------
def test_refusals_are_error_codes_not_launches(lib):
    M, N, K = 300, 320, 128
    Aq, Wq, ws, b = R.exact_operands(M, N, K, 91, DEV)
    Ab = torch.zeros(M, K + 48, dtype=torch.uint8, device=DEV)
    Wb = torch.zeros(N, K + 32, dtype=torch.uint8, device=DEV)
    out = torch.full((M + 8, N + 64), 1.0, device=DEV)                         # fp32: wide enough for every output type
    res, o2 = torch.zeros(M, N + 16, device=DEV), torch.zeros(M, 2 * N, dtype=torch.bfloat16, device=DEV)
    cs, sn = torch.zeros(M, 32, device=DEV), torch.zeros(M, 32, device=DEV)
    ok = dict(A=Ab, lda=K + 48, W=Wb, ldw=K + 32, bias=b, out=out, ldo=N + 24, M=M, N=N, K=K)
    rope = dict(rope_cos=cs, rope_sin=sn, rope_rows_per_batch=100, rope_cols=128)
    S, A = hip.ERR_SHAPE, hip.ERR_ARG
    cases = [
        (0, dict(K=64), S), (0, dict(K=0), S), (0, dict(M=0), S), (0, dict(N=N + 8), S),
        (0, dict(lda=K + 8), S), (0, dict(lda=K - 16), S), (0, dict(ldw=K + 8), S), (0, dict(ldw=K - 16), S),
        (0, dict(w_rows=-1), S), (0, dict(w_rows=N + 1), S),
        (0, dict(ldo=N - 8), S), (0, dict(ldo=N + 4), S), (4, dict(ldo=N - 4), S), (4, dict(ldo=N + 2), S), (1, dict(ldo=N + 2), S),
        (5, dict(ldo=N // 2 - 8), S), (5, dict(ldo=N // 2 + 4), S), (2, dict(ldo=N + 4, **rope), S),
        (1, dict(residual=res, ldr=N - 4), S), (1, dict(residual=res, ldr=N + 2), S),
        (1, dict(residual=res, ldr=N + 16, out2_bf16=o2, ldo2=N - 4), S), (1, dict(residual=res, ldr=N + 16, out2_bf16=o2, ldo2=N + 2), S),
        (2, dict(), A), (2, dict(rope, rope_cos=None), A), (2, dict(rope, rope_sin=None), A),
        (2, dict(rope, N=N - 16, ldo=N + 24), S), (2, dict(rope, rope_cols=96), S), (2, dict(rope, rope_cols=N + 64), S),
        (2, dict(rope, rope_cols=-64), S), (2, dict(rope, rope_rows_per_batch=0), S),
        (5, dict(bias=None), A), (5, dict(N=N - 16), S),
        (0, dict(A=None), A), (0, dict(W=None), A), (0, dict(out=None), A),
    ] + [(e, dict(rope, rope_pos=torch.zeros(M, dtype=torch.int32, device=DEV), out2_bf16=o2, ldo2=2 * N), A) for e in (3, 6, 7, 8, 9, -1, 10)]
    for epi, change, code in cases:
        got = launch(lib, epi, ws, rc_only=True, **{**ok, **change})
        assert got == (code, 0), (epi, {k: v for k, v in change.items() if not isinstance(v, torch.Tensor)}, got)
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())
    assert launch(lib, 0, ws, rc_only=True, **ok) == (hip.OK, 256)             # and the unchanged arguments do launch
    torch.cuda.synchronize()
    assert not bool((out == 1.0).all())


# ------------------------------------------------------- the fp8 LayerNorm and the row quantiser -------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("d", [64, 256, 320, 768, 1024, 1472, 2048])
def test_layernorm_fp8_elementwise(lib, d, affine):
    """one to eight float4 chunks per lane (320, 768 and 1472 with a partial last chunk); M in {1, 5, 70} plus one constant row
    (variance 0); with gamma, every eighth column is scaled 400 so that those outputs saturate, and a last launch scales the whole
    gamma of one row.  Rows after M of the sentinel-filled output stay intact."""
    worst, saturating = 0.0, 0
    runs = [(M, 1.0) for M in (1, 5, 70)] + ([(1, 400.0)] if affine else [])
    for M, gscale in runs:
        x, g, b = (t.to(DEV) for t in R.layernorm_data(M, d, 71 + M))
        g = g * gscale
        rows = M + 1 if gscale == 1.0 else 1
        x = x[:rows].contiguous()
        keep = x.clone()
        out = torch.full((rows + 8, d), U8_SENT, dtype=torch.uint8, device=DEV)
        hip.check(lib.ditto_layernorm_fp8(x.data_ptr(), g.data_ptr() if affine else None, b.data_ptr() if affine else None,
                                          out.data_ptr(), rows, d, stream()))
        torch.cuda.synchronize()
        assert bool((out[rows:] == U8_SENT).all()) and torch.equal(x, keep)
        want, e = R.layernorm(x, g if affine else None, b if affine else None)
        saturating += int((want.abs() > 448).sum())
        worst = max(worst, R.worst_ratio(R.deq(out[:rows]), want, e, stored="e4m3"))
    assert saturating >= 32 or not affine, saturating
    report(f"layernorm/d{d}/{'affine' if affine else 'plain'}", worst)


@pytest.mark.parametrize("rows,cols", [(1, 4), (5, 132), (200, 384), (7, 1028)])
def test_quantize_rows_fp8_elementwise(lib, rows, cols):
    x = R.quantize_data(rows, cols, 81).to(DEV)
    keep = x.clone()
    q = torch.full((rows + 8, cols), U8_SENT, dtype=torch.uint8, device=DEV)
    sc = torch.full((rows + 8,), 7.0, device=DEV)
    hip.check(lib.ditto_quantize_rows_fp8(x.data_ptr(), rows, cols, q.data_ptr(), sc.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert bool((q[rows:] == U8_SENT).all() and (sc[rows:] == 7.0).all()) and torch.equal(x, keep)
    q, sc = q[:rows], sc[:rows]
    assert not bool(((q & 0x7F) == 0x7F).any())                 # no NaN byte
    amax = x.double().abs().amax(dim=1)
    want_sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert bool(((sc.double() - want_sc).abs() <= R.ulp32(want_sc)).all())
    dq = R.deq(q)
    idx = x.abs().argmax(dim=1, keepdim=True)
    nz = amax > 0
    assert torch.equal(dq.gather(1, idx)[nz], 448.0 * torch.sign(x.double().gather(1, idx))[nz])   # the maximal element: exactly +-448
    if rows >= 5:
        assert float(sc[1]) == 1.0 and bool((q[1] == 0).all())                 # the all-zero row
        assert int(idx[2]) == cols - 1 and float(dq[2, -1]) == -448.0           # a negative maximum in the last column
        rest = torch.cat([dq[3, :1], dq[3, 2:]]).abs()
        assert float(rest.max()) < 2.0 ** -4 and bool((rest == 0).any()) and bool(((rest > 0) & (rest < 2.0 ** -6)).any())
    err, bound = R.quantize_bound(x, q, sc)
    report(f"quantize/{rows}x{cols}", float((err / bound).max()))
