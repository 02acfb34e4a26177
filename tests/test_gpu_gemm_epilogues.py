"""Every fused epilogue of the bf16 GEMM family at kernel level, per tile structure, against the fp64 references and the derived
elementwise bounds of gemm_epi_ref.py (ditto_gemm_epilogue_bf16: every epilogue, every stride).  Every value assertion is
elementwise (worst_ratio <= 1) or bitwise.  -s prints the worst ratio of each case.

The entry reports the structure that ran, and every case asserts it.  Pairs that fall back BY DESIGN (csrc/gemm.hip launch_gemm):
gemm_tile 192 runs epilogues 0 / 1 / 4 only, so 2 / 3 forced to 192 run the 128 x 128 kernel; epilogue 6 exists on 127 / 128 / 256
and epilogue 9 on 127 / 128 / 256: any other forced tile takes the automatic rule for them; epilogues 7 and 8 exist on the
256 x 256 kernel only and run there whatever is forced.  No (shape, structure) pair of these tests is refused by launch_gemm; the
refusals that exist (epilogue 5, epilogue 7 outside the fused rule, N % 256 for 7 / 8) are asserted by error code below."""
import contextlib
import ctypes as C
import math

import pytest
import torch

import gemm_epi_ref as R
from ditto_tts_amd import hip
from gpu_util import asym, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF_SENT, F32_SENT = 0x7FC1, 0x7FC00001
# (gemm_tile, gemm_flags): deep 128 x 128, 128 x 128, 256 x 128 ring, 128 x 256 ping-pong, 256 x 192, 256 x 256 with the
# straight-line epilogue / the general epilogue / the tile-switch K loop
STRUCTS = [(127, 321), (128, 321), (129, 321), (131, 321), (192, 321), (256, 321), (256, 321 + 1024), (256, 321 + 16384)]
SID = [f"tile{t}-flags{f}" for t, f in STRUCTS]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return hip.lib()


@contextlib.contextmanager
def forced(lib, tile, flags):
    hip.check(lib.ditto_set_option(b"gemm_tile", tile))
    hip.check(lib.ditto_set_option(b"gemm_flags", flags))
    try:
        yield
    finally:
        hip.check(lib.ditto_set_option(b"gemm_tile", 0))
        hip.check(lib.ditto_set_option(b"gemm_flags", 321))


def expected_structure(tile, epi):
    """the structure launch_gemm takes for a forced tile; None = the automatic rule decides (fallback by design)"""
    if epi in (7, 8):
        return 256
    if epi in (6, 9) and tile not in (127, 128, 256):
        return None
    if tile == 192 and epi not in (0, 1, 4):
        return 128
    return tile


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + off


def launch(lib, epi, tile=None, rc_only=False, **kw):
    """one launch; returns the structure that ran (asserted against the forced tile when given)"""
    a = hip.GemmEpilogueArgs()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    st = C.c_int(-1)
    rc = lib.ditto_gemm_epilogue_bf16(C.byref(a), epi, C.byref(st), stream())
    if rc_only:
        return rc, st.value
    hip.check(rc)
    if tile is not None:
        want = expected_structure(tile, epi)
        assert st.value == want or (want is None and st.value in (127, 128, 256)), (tile, epi, st.value)
    return st.value


_cache = {}


def cached(key, fn):
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        _cache[key] = fn()
    return _cache[key]


def rope_case(M, d, seed=11):
    def make():
        N, K = 3 * d, d
        A, W, b = R.operands(M, N, K, seed, DEV)
        pre, absacc = R.linear(A, W, b)
        return A, W, b, pre, R.acc_bound(absacc, K)
    return cached(("rope", M, d, seed), make)


def rope_tables(positions):
    invf = R.inv_freq().to(DEV)
    cs, sn = R.tables(invf, positions)
    return invf, R.freq_rev(invf).contiguous(), cs, sn


# ------------------------------------------------------- a. QKV + RoPE, dense -------------------------------------------------------
ROPE_SHAPES = [(768, 1024, 4096), (768, 200, 1000), (768, 333, 999), (768, 4096, 4396), (320, 300, 600), (1024, 512, 1024),
               (256, 256, 512), (256, 64, 1), (256, 64, 63)]


@pytest.mark.parametrize("struct", STRUCTS, ids=SID)
@pytest.mark.parametrize("d,rpb,M", ROPE_SHAPES)
def test_qkv_rope_dense(lib, d, rpb, M, struct):
    tile, flags = struct
    N, K, rc = 3 * d, d, 2 * d
    A, W, b, pre, accb = rope_case(M, d)
    invf, frev, cs, sn = rope_tables(max(M, rpb))          # tables cover every row index, not only every position

    def refs():
        pos = torch.arange(M, device=DEV) % rpb
        c64, s64 = R.rope_exact_tables(invf, pos)
        free = R.rope(pre, torch.arange(M, device=DEV), rc, c64, s64)
        return (free, R.rope_bound(pre, accb, rc, R.dtheta_table_free(pos, invf), R.E_SINCOS), R.rope(pre, pos, rc, cs, sn),
                R.rope_bound(pre, accb, rc), R.rope_bound(pre, torch.zeros_like(accb), rc, None, R.G))   # last: the tables' own rounding
    want_free, bound_free, want_tab, bound_tab, tab_round = cached(("ropewant", d, rpb, M), refs)
    common = dict(A=A, lda=K, W=W, bias=b, ldo=N, M=M, N=N, K=K)
    rope = dict(rope_cos=cs, rope_sin=sn, rope_rows_per_batch=rpb, rope_cols=rc)
    with forced(lib, tile, flags):
        def run(epi, **kw):
            out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            launch(lib, epi, tile, out=out, **common, **kw)
            return out
        free, tab, plain = run(2, rope_freq_rev=frev, **rope), run(2, **rope), run(0)
        free2, tab2 = run(2, rope_freq_rev=frev, **rope), run(2, **rope)
    r_free = R.worst_ratio(free, want_free, bound_free, stored_bf16=True)
    r_tab = R.worst_ratio(tab, want_tab, bound_tab, stored_bf16=True)
    # the two paths against each other: both angle terms (table: 0) and both results' value bounds and stores
    r_x = R.worst_ratio(free, tab.double(), bound_free + bound_tab + tab_round + 2.0 ** -8 * tab.double().abs(), stored_bf16=True)
    print(f"rope d {d} rpb {rpb} M {M} {tile}/{flags}: table-free {r_free:.3f} table {r_tab:.3f} cross {r_x:.3f}")
    assert r_free <= 1.0 and r_tab <= 1.0 and r_x <= 1.0
    assert torch.equal(free[:, rc:], plain[:, rc:]) and torch.equal(tab[:, rc:], plain[:, rc:])   # v columns: epilogue 0's bits
    assert torch.equal(free, free2) and torch.equal(tab, tab2)


@pytest.mark.parametrize("struct", STRUCTS, ids=SID)
def test_qkv_rope_pairing_and_sign_bit_for_bit(lib, struct):
    """One-hot weight rows and no bias: acc[r][c] = A[r][k(c)] exactly, distinct per column of a row.  Tables with (cos, sin) =
    (0, 1) at odd positions and (1, 0) at even ones: the output is (-hi, lo) respectively (lo, hi), bit for bit."""
    tile, flags = struct
    d, rpb, M = 320, 150, 450
    N, K, rc = 3 * d, d, 2 * d
    A = asym((M, K), 61).to(torch.bfloat16).to(DEV)
    perm = (torch.arange(N) * 7 + 3) % K                      # column c reads A[:, perm[c]]: the partners (c, c + 32) differ
    W = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    W[torch.arange(N), perm] = 1.0
    acc = A[:, perm.to(DEV)]                                  # bf16, exact
    odd = (torch.arange(max(M, rpb), device=DEV) % 2 == 1).float()[:, None].expand(-1, 32).contiguous()
    cs, sn = (1 - odd).contiguous(), odd
    pos = torch.arange(M, device=DEV) % rpb
    lo, hi = R._split(acc, rc)
    o = (pos % 2 == 1)[:, None, None]
    want = R._join(torch.where(o, -hi, lo), torch.where(o, lo, hi), acc[:, rc:])
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    with forced(lib, tile, flags):
        launch(lib, 2, tile, A=A, lda=K, W=W, out=out, ldo=N, M=M, N=N, K=K, rope_cos=cs, rope_sin=sn, rope_rows_per_batch=rpb,
               rope_cols=rc)
    bad = (out.view(torch.int16) != want.contiguous().view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"first wrong (row, col): {bad[0].tolist()} of {bad.shape[0]}"


# ------------------------------------------------------- b. QKV + RoPE, packed -------------------------------------------------------
PACKED_STRUCTS = [s for s in STRUCTS if s[0] in (127, 128, 256)]


def _packed_pos(kind, M):
    if kind == "cu_seqlens":
        lens = [1, 63, 64, 65, 200, 1000]
        assert sum(lens) == M
        return torch.cat([torch.arange(n) for n in lens]).int()
    g = torch.Generator().manual_seed(9)
    return torch.randperm(M, generator=g).int()               # not monotone: nothing but rope_pos[row] can give these angles


@pytest.mark.parametrize("struct", PACKED_STRUCTS, ids=[f"tile{t}-flags{f}" for t, f in PACKED_STRUCTS])
@pytest.mark.parametrize("kind", ["cu_seqlens", "permutation"])
def test_qkv_rope_packed(lib, kind, struct):
    tile, flags = struct
    d, M = 768, 1393
    N, K, rc = 3 * d, d, 2 * d
    A, W, b, pre, accb = rope_case(M, d, seed=17)
    invf, frev, cs, sn = rope_tables(M)
    pos = _packed_pos(kind, M).to(DEV)
    # rope_pos = the last M ints before a guard region of 0x7fffffff (readable memory; only the table-free launch sees it)
    buf = torch.full((M + 4096,), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    buf[:M] = pos
    posl = pos.long()
    c64, s64 = R.rope_exact_tables(invf, posl)
    rows = torch.arange(M, device=DEV)
    common = dict(A=A, lda=K, W=W, bias=b, ldo=N, M=M, N=N, K=K, rope_cos=cs, rope_sin=sn, rope_cols=rc)
    with forced(lib, tile, flags):
        free = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        launch(lib, 9, tile, out=free, rope_pos=buf, rope_freq_rev=frev, **common)
        tab = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        launch(lib, 9, tile, out=tab, rope_pos=pos.contiguous(), **common)
    r_free = R.worst_ratio(free, R.rope(pre, rows, rc, c64, s64),
                           R.rope_bound(pre, accb, rc, R.dtheta_table_free(posl, invf), R.E_SINCOS), stored_bf16=True)
    r_tab = R.worst_ratio(tab, R.rope(pre, posl, rc, cs, sn), R.rope_bound(pre, accb, rc), stored_bf16=True)
    print(f"packed {kind} {tile}/{flags}: table-free {r_free:.3f} table {r_tab:.3f}")
    assert r_free <= 1.0 and r_tab <= 1.0
    assert bool((buf[M:] == 0x7FFFFFFF).all())


@pytest.mark.parametrize("struct", PACKED_STRUCTS, ids=[f"tile{t}-flags{f}" for t, f in PACKED_STRUCTS])
@pytest.mark.parametrize("free", [True, False], ids=["table-free", "tables"])
def test_qkv_rope_packed_is_bitwise_the_dense_epilogue(lib, struct, free):
    """rope_pos[r] = r % rpb: the same float position, the padded layout's bits (csrc/gemm_common.h)"""
    tile, flags = struct
    d, rpb, M = 768, 200, 1000
    N, K, rc = 3 * d, d, 2 * d
    A, W, b, _, _ = rope_case(M, d)
    invf, frev, cs, sn = rope_tables(M)
    pos = (torch.arange(M, device=DEV) % rpb).int()
    common = dict(A=A, lda=K, W=W, bias=b, ldo=N, M=M, N=N, K=K, rope_cos=cs, rope_sin=sn, rope_cols=rc)
    if free:
        common["rope_freq_rev"] = frev
    o2, o9 = (torch.zeros(M, N, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    with forced(lib, tile, flags):
        launch(lib, 2, tile, out=o2, rope_rows_per_batch=rpb, **common)
        launch(lib, 9, tile, out=o9, rope_pos=pos, **common)
    assert torch.equal(o2, o9)


# ------------------------------------------------- c. the model's split QKV launch -------------------------------------------------
@pytest.mark.parametrize("M", [8192, 600])
def test_split_qkv_launch_is_bitwise_the_single_launch(lib, M):
    """csrc/ditto_api.hip "qkv_split": all but the last 256 columns with epilogue 2, the last 256 (v) columns as a second launch with
    epilogue 0 through offset W / bias / out pointers and ldo = 3 d."""
    d, rpb = 768, 1024
    N, K, rc, Nm = 3 * d, d, 2 * d, 3 * d - 256
    A, W, b = R.operands(M, N, K, 23, DEV)
    invf, frev, cs, sn = rope_tables(max(M, rpb))
    rope = dict(rope_cos=cs, rope_sin=sn, rope_rows_per_batch=rpb, rope_cols=rc, rope_freq_rev=frev)
    one, two = (torch.zeros(M, N, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    launch(lib, 2, A=A, lda=K, W=W, bias=b, out=one, ldo=N, M=M, N=N, K=K, **rope)
    st_main = launch(lib, 2, A=A, lda=K, W=W, bias=b, out=two, ldo=N, M=M, N=Nm, K=K, **rope)
    launch(lib, 0, A=A, lda=K, W=_ptr(W, Nm * K * 2), bias=_ptr(b, Nm * 4), out=_ptr(two, Nm * 2), ldo=N, M=M, N=256, K=K)
    if M == 8192:
        assert st_main == 256                                  # the shape where the model's rule fires: 32 x 8 tiles of 256 x 256
    assert torch.equal(one, two)


# --------------------------------------------- d. strides and guard bands, every epilogue ---------------------------------------------
TOP, BELOW = 4, 260


def _window(M, width, ld, f32=False):
    """[TOP + M + BELOW, ld] filled with the sentinel; the launch writes rows TOP .. TOP + M, columns < width"""
    dt, s = (torch.int32, F32_SENT) if f32 else (torch.int16, BF_SENT)
    buf = torch.full((TOP + M + BELOW, ld), s, dtype=dt, device=DEV)
    return buf, buf.view(torch.float32 if f32 else torch.bfloat16)


def _guards_intact(buf, M, width, f32=False):
    s = F32_SENT if f32 else BF_SENT
    return bool((buf[:TOP] == s).all() and (buf[TOP + M:] == s).all() and (buf[TOP:TOP + M, width:] == s).all())


def _strided_operands(M, N, K, seed, bias=True):
    """A at lda = K + 8 and W at ldw = K + 64 with NaN in every element the kernel must not use: the pad columns, and the W rows
    from w_rows = N - 64 on.  Returns the buffers and the plain (valid) operands."""
    A, W, b = R.operands(M, N, K, seed, DEV, bias=bias)
    w_rows = N - 64
    Ab = torch.full((M, K + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    Ab[:, :K] = A
    Wb = torch.full((N, K + 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    Wb[:w_rows, :K] = W[:w_rows]
    return Ab, Wb, A, W, b, w_rows


PLAIN_SHAPES = [(300, 144, 64), (513, 272, 192), (777, 320, 128), (300, 2336, 128)]


@pytest.mark.parametrize("struct", STRUCTS, ids=SID)
@pytest.mark.parametrize("M,N,K", PLAIN_SHAPES)
@pytest.mark.parametrize("epi", [0, 1, 4, 6])
def test_strides_and_guard_bands_plain(lib, epi, M, N, K, struct):
    tile, flags = struct
    Ab, Wb, A, W, b, w_rows = _strided_operands(M, N, K, 31)
    pre, absacc = R.linear(A, W, b)
    accb = R.acc_bound(absacc, K)
    f32 = epi in (1, 4)
    ldo = N + 24
    buf, view = _window(M, N, ldo, f32)
    kw = dict(A=Ab, lda=K + 8, W=Wb, ldw=K + 64, w_rows=w_rows, bias=b, out=view[TOP:], ldo=ldo, M=M, N=N, K=K)
    side_copy = epi == 1 and M == 513                      # (a side copy keeps a tile off the straight-line epilogue)
    if epi == 1:
        ldr = N + 12
        res = torch.full((M, ldr), float("nan"), device=DEV)
        res[:, :N] = asym((M, N), 37).to(DEV)
        b2, v2 = _window(M, N, N + 4)
        kw.update(residual=res, ldr=ldr)
        if side_copy:
            kw.update(out2_bf16=v2[TOP:], ldo2=N + 4)
    with forced(lib, tile, flags):
        launch(lib, epi, tile, **kw)
    got = view[TOP:TOP + M, :w_rows]
    assert _guards_intact(buf, M, N, f32)
    if epi == 1:
        want = pre + res[:, :N].double()
        r = R.worst_ratio(got, want[:, :w_rows], (accb + 2 * R.G * want.abs())[:, :w_rows])
        if side_copy:
            assert _guards_intact(b2, M, N)
            assert torch.equal(v2[TOP:TOP + M, :w_rows], got.to(torch.bfloat16))   # the bf16 side copy: the fp32 result, rounded
    elif epi == 4:
        r = R.worst_ratio(got, pre[:, :w_rows], accb[:, :w_rows])
    else:
        want = pre.clamp_min(0) if epi == 6 else pre
        r = R.worst_ratio(got, want[:, :w_rows], accb[:, :w_rows], stored_bf16=True)
    print(f"epilogue {epi} M {M} N {N} K {K} {tile}/{flags}: {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("struct", STRUCTS, ids=SID)
@pytest.mark.parametrize("M,N,K", [(300, 320, 64), (513, 2336, 192), (777, 1088, 128)])
def test_strides_and_guard_bands_gated(lib, M, N, K, struct):
    """epilogue 3 against gelu_erf * sigmoid itself, on each structure"""
    tile, flags = struct
    Ab, Wb, A, W, b, w_rows = _strided_operands(M, N, K, 41)
    pre, absacc = R.linear(A, W, b)
    accb = R.acc_bound(absacc, K)
    ldo, valid = N // 2 + 24, w_rows // 32 * 16
    buf, view = _window(M, N // 2, ldo)
    with forced(lib, tile, flags):
        launch(lib, 3, tile, A=Ab, lda=K + 8, W=Wb, ldw=K + 64, w_rows=w_rows, bias=b, out=view[TOP:], ldo=ldo, M=M, N=N, K=K)
    assert _guards_intact(buf, M, N // 2)
    r = R.worst_ratio(view[TOP:TOP + M, :valid], R.gated(pre)[:, :valid], R.gated_bound(pre, accb)[:, :valid], stored_bf16=True)
    print(f"gated M {M} N {N} K {K} {tile}/{flags}: {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("struct", STRUCTS, ids=SID)
@pytest.mark.parametrize("M,N,K,rc", [(300, 320, 64, 192), (513, 2368, 192, 1600), (777, 320, 128, 128)])
@pytest.mark.parametrize("epi", [2, 9])
def test_strides_and_guard_bands_rope(lib, epi, M, N, K, rc, struct):
    tile, flags = struct
    if epi == 9 and tile not in (127, 128, 256):
        tile = 0                                               # epilogue 9 elsewhere: the automatic rule (asserted by `launch`)
    Ab, Wb, A, W, b, w_rows = _strided_operands(M, N, K, 51)
    pre, absacc = R.linear(A, W, b)
    accb = R.acc_bound(absacc, K)
    rpb = 211
    invf, frev, cs, sn = rope_tables(max(M, rpb))
    pos = torch.arange(M, device=DEV) % rpb
    ldo = N + 24
    kw = dict(A=Ab, lda=K + 8, W=Wb, ldw=K + 64, w_rows=w_rows, bias=b, ldo=ldo, M=M, N=N, K=K, rope_cos=cs, rope_sin=sn,
              rope_cols=rc)
    kw.update(dict(rope_rows_per_batch=rpb) if epi == 2 else dict(rope_pos=pos.int().contiguous()))
    c64, s64 = R.rope_exact_tables(invf, pos)
    rows = torch.arange(M, device=DEV)
    want = {True: R.rope(pre, rows, rc, c64, s64), False: R.rope(pre, pos, rc, cs, sn)}
    bound = {True: R.rope_bound(pre, accb, rc, R.dtheta_table_free(pos, invf), R.E_SINCOS), False: R.rope_bound(pre, accb, rc)}
    for free in (True, False):
        buf, view = _window(M, N, ldo)
        with forced(lib, tile, flags):
            launch(lib, epi, struct[0], out=view[TOP:], **kw, **(dict(rope_freq_rev=frev) if free else {}))
        assert _guards_intact(buf, M, N)
        r = R.worst_ratio(view[TOP:TOP + M, :w_rows], want[free][:, :w_rows], bound[free][:, :w_rows], stored_bf16=True)
        print(f"rope epilogue {epi} M {M} N {N} K {K} {struct[0]}/{flags} table-free {free}: {r:.3f}")
        assert r <= 1.0


FLAGS256 = [321, 321 + 1024, 321 + 16384]


@pytest.mark.parametrize("flags", FLAGS256)
@pytest.mark.parametrize("M,N,K", [(300, 512, 64), (513, 768, 192)])
def test_strides_and_guard_bands_gated_pre(lib, M, N, K, flags):
    Ab, Wb, A, W, b, w_rows = _strided_operands(M, N, K, 43)
    pre, absacc = R.linear(A, W, b)
    accb = R.acc_bound(absacc, K)
    ldo, ldo2, valid = N // 2 + 24, N + 24, w_rows // 32 * 16
    buf, view = _window(M, N // 2, ldo)
    b2, v2 = _window(M, N, ldo2)
    with forced(lib, 128, flags):                              # (forced elsewhere: epilogue 8 still runs the 256 x 256 kernel)
        launch(lib, 8, 128, A=Ab, lda=K + 8, W=Wb, ldw=K + 64, w_rows=w_rows, bias=b, out=view[TOP:], ldo=ldo, out2_bf16=v2[TOP:],
               ldo2=ldo2, M=M, N=N, K=K)
    assert _guards_intact(buf, M, N // 2) and _guards_intact(b2, M, N)
    r = R.worst_ratio(view[TOP:TOP + M, :valid], R.gated(pre)[:, :valid], R.gated_bound(pre, accb)[:, :valid], stored_bf16=True)
    r2 = R.worst_ratio(v2[TOP:TOP + M, :2 * valid], pre[:, :2 * valid], accb[:, :2 * valid], stored_bf16=True)
    print(f"gated_pre M {M} N {N} K {K} flags {flags}: out {r:.3f} pre {r2:.3f}")
    assert r <= 1.0 and r2 <= 1.0


def _bwd_case(M, F, K, seed):
    def make():
        A, W, _ = R.operands(M, F, K, seed, DEV, bias=False)
        pre = (1.5 * asym((M, 2 * F), seed + 3)).to(torch.bfloat16).to(DEV)
        dact, absacc = R.linear(A, W)
        return A, W, pre, dact, R.acc_bound(absacc, K)
    return cached(("bwd", M, F, K, seed), make)


def _check_bwd(lib, M, F, K, flags, strided):
    A, W, pre, dact, accb = _bwd_case(M, F, K, 71)
    lda, ldw, ldpre, ldo = (K + 8, K + 64, 2 * F + 16, 2 * F + 24) if strided else (K, K, 2 * F, 2 * F)
    w_rows = F - 64 if strided else F
    Ab = torch.full((M, lda), float("nan"), dtype=torch.bfloat16, device=DEV)
    Ab[:, :K] = A
    Wb = torch.full((F, ldw), float("nan"), dtype=torch.bfloat16, device=DEV)
    Wb[:w_rows, :K] = W[:w_rows]
    Pb = torch.full((M, ldpre), float("nan"), dtype=torch.bfloat16, device=DEV)
    Pb[:, :2 * F] = pre
    buf, view = _window(M, 2 * F, ldo)
    prow = 2 * ((M + 255) // 256)
    part = torch.full((prow + 4, 2 * F), F32_SENT, dtype=torch.int32, device=DEV)
    with forced(lib, 0, flags):
        launch(lib, 7, 0, A=Ab, lda=lda, W=Wb, ldw=ldw, w_rows=w_rows, out=view[TOP:], ldo=ldo, pre_bf16=Pb, ldpre=ldpre,
               colsum_partial=part.view(torch.float32), M=M, N=F, K=K)
    assert _guards_intact(buf, M, 2 * F)
    assert bool((part[prow:] == F32_SENT).all())
    got = view[TOP:TOP + M, :2 * F]
    v = 2 * w_rows
    r = R.worst_ratio(got[:, :v], R.gated_bwd(dact, pre)[:, :v], R.gated_bwd_bound(dact, accb, pre)[:, :v], stored_bf16=True)
    # each partial row = the fp32 sum, in any order, of the ROUNDED outputs of its own 128 rows; rows past M add exactly nothing
    s, sa = R.colsum_partials(got[:, :v], M)
    p = part.view(torch.float32)[:prow, :v].double()
    worst = float(((p - s).abs() - 128 * R.G * sa).max())
    assert bool(torch.isfinite(p).all()) and worst <= 0.0, worst
    if M % 256 and M % 256 <= 128:
        assert bool((part.view(torch.float32)[prow - 1, :v] == 0.0).all())       # the last half tile owns no valid row
    return r


@pytest.mark.parametrize("flags", FLAGS256)
def test_strides_and_guard_bands_gated_bwd(lib, flags):
    r = _check_bwd(lib, 2916, 3072, 192, flags, strided=True)
    print(f"gated_bwd strided flags {flags}: {r:.3f}")
    assert r <= 1.0


# ------------------------------------------- e. the training epilogues on the 256 x 256 kernel -------------------------------------------
@pytest.mark.parametrize("flags", FLAGS256)
@pytest.mark.parametrize("M", [4000, 4096])
def test_gated_pre_is_the_gated_epilogue_plus_the_preactivations(lib, M, flags):
    N, K = 6144, 768
    A, W, b = cached(("pre", M), lambda: R.operands(M, N, K, 81, DEV))
    pre, absacc = R.linear(A, W, b)
    o3, o8 = (torch.zeros(M, N // 2, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    o2 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    with forced(lib, 256, flags):
        launch(lib, 3, 256, A=A, lda=K, W=W, bias=b, out=o3, ldo=N // 2, M=M, N=N, K=K)
        launch(lib, 8, 256, A=A, lda=K, W=W, bias=b, out=o8, ldo=N // 2, out2_bf16=o2, ldo2=N, M=M, N=N, K=K)
    assert torch.equal(o3, o8)
    r = R.worst_ratio(o2, pre, R.acc_bound(absacc, K), stored_bf16=True)
    r3 = R.worst_ratio(o3, R.gated(pre), R.gated_bound(pre, R.acc_bound(absacc, K)), stored_bf16=True)
    print(f"gated_pre M {M} flags {flags}: pre {r:.3f} gated {r3:.3f}")
    assert r <= 1.0 and r3 <= 1.0


@pytest.mark.parametrize("flags", FLAGS256)
@pytest.mark.parametrize("M", [3072, 2916])
def test_gated_bwd_values_and_column_sums(lib, M, flags):
    r = _check_bwd(lib, M, 3072, 768, flags, strided=False)
    print(f"gated_bwd M {M} flags {flags}: {r:.3f}")
    assert r <= 1.0


def test_refusals_are_error_codes_not_launches(lib):
    M, F, K = 512, 3072, 64
    A, W, _ = R.operands(M, F, K, 91, DEV, bias=False)
    pre = torch.zeros(M, 2 * F, dtype=torch.bfloat16, device=DEV)
    out = torch.full((M, 2 * F), 1.0, dtype=torch.bfloat16, device=DEV)
    part = torch.zeros(4, 2 * F, device=DEV)
    kw = dict(A=A, lda=K, W=W, out=out, ldo=2 * F, pre_bf16=pre, ldpre=2 * F, colsum_partial=part, M=M, K=K)
    assert launch(lib, 7, rc_only=True, N=F, **kw) == (hip.ERR_SHAPE, 0)               # 24 tiles: outside the fused rule
    assert launch(lib, 7, rc_only=True, N=F - 128, **kw) == (hip.ERR_SHAPE, 0)         # N % 256
    b = torch.zeros(F, device=DEV)
    assert launch(lib, 8, rc_only=True, N=F - 128, bias=b, out2_bf16=pre, ldo2=2 * F, **kw) == (hip.ERR_SHAPE, 0)
    assert launch(lib, 5, rc_only=True, N=F, bias=b, **kw) == (hip.ERR_ARG, 0)
    assert launch(lib, 2, rc_only=True, N=F, **kw) == (hip.ERR_ARG, 0)                 # no tables
    assert launch(lib, 0, rc_only=True, N=F, **{**kw, "lda": K + 4}) == (hip.ERR_SHAPE, 0)
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())
