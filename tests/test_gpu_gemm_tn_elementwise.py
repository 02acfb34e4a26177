"""The weight-gradient GEMM (csrc/gemm_tn.hip through ditto_gemm_tn_bf16) elementwise against the fp64 reference and the derived
bound of gemm_tn_ref.py, on all three kernels, at the smallest shapes where each of them can go wrong (gemm_tn_ref.SHAPES, KS,
SPLITS: ragged tiles on both tile sizes, K-tile counts 1..7 and 10, whole K-tiles next to K-crossing ones, uneven and empty
splits) and on the model's operand strides (gemm_tn_ref.LAYOUTS).

Every operand is a window of a NaN-filled buffer with guard rows above and below: nothing outside [K, width] may contribute, so one
read of row K, of a guard column or of a row at the wrong stride puts a NaN into the output, which no element may hold.  The output
is a window of a buffer of F32_SENT words (ldo > No without splits; guard rows with), the workspace is exactly the bytes the entry
asks for inside a larger 0xA5-filled allocation: every word outside the output window and every byte outside the workspace must
come back as it was.  `real` operands: worst_ratio <= 1 over every element.  `exact` operands (non-zero integers, every partial sum
exact in fp32): torch.equal with the reference, hence with every other kernel and split count.  Every case runs twice, bit-equal.
-s prints the worst ratio per kernel and shape.  test_gemm_tn_bound.py shows what these assertions refuse."""
import contextlib

import pytest
import torch

import gemm_tn_ref as T
from ditto_tts_amd import hip
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_SENT = 0x7FC00001
WS_FILL, WS_PAD = 0xA5, 4096
# name: (tile argument, gemm_flags)
KERNELS = {"ring": (128, 321), "two_buffer": (128, 321 + 2048), "wide": (256, 321)}


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


_pools = {}


def dev_pool(family, seed):
    if (family, seed) not in _pools:
        _pools[(family, seed)] = T.pool(family, seed).to(DEV)
    return _pools[(family, seed)]


_refs = {}


def case(family, Mo, No, K, lay):
    """operands and reference of one case, computed once and shared by the three kernels and the five split counts"""
    key = (family, Mo, No, K, lay)
    if key not in _refs:
        if any(k[1:3] != (Mo, No) for k in _refs):       # the tests come shape by shape: keep one shape's cases
            _refs.clear()
        xb, xv, ldx, yb, yv, ldy = T.operands(family, Mo, No, K, lay, pools=dev_pool)
        want, absacc = T.reference(xv[:K], yv[:K])
        _refs[key] = (xb, xv, ldx, yb, yv, ldy, want, absacc)
    return _refs[key]


def out_window(Mo, No, S):
    """(int32 buffer of sentinels, row offset, column offset, ldo)"""
    ldo, col = (No, 0) if S > 1 else (No + 12, 4)
    buf = torch.full((T.GUARD_BEFORE + Mo + T.GUARD_AFTER, ldo), F32_SENT, dtype=torch.int32, device=DEV)
    return buf, T.GUARD_BEFORE, col, ldo


def workspace(Mo, No, S):
    need = 256 + (S * Mo * No * 4 if S > 1 else 0)
    raw = torch.full((256 + need + WS_PAD,), WS_FILL, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 256 == 0
    return raw, need


def run(lib, tile, xv, ldx, yv, ldy, Mo, No, K, S):
    """one launch into fresh guarded buffers -> the [Mo, No] fp32 result; asserts every guard"""
    obuf, r0, c0, ldo = out_window(Mo, No, S)
    raw, need = workspace(Mo, No, S)
    optr = obuf.data_ptr() + (r0 * ldo + c0) * 4
    hip.check(lib.ditto_gemm_tn_bf16(xv.data_ptr(), ldx, yv.data_ptr(), ldy, optr, ldo, Mo, No, K, S, tile,
                                     raw.data_ptr() + 256, need, stream()))
    win = obuf[r0:r0 + Mo, c0:c0 + No].clone()
    obuf[r0:r0 + Mo, c0:c0 + No] = F32_SENT
    assert bool((obuf == F32_SENT).all()), "a word outside the output window was written"
    assert bool((raw[:256] == WS_FILL).all()) and bool((raw[256 + need:] == WS_FILL).all()), "a byte outside the workspace was written"
    return win.view(torch.float32)


@pytest.mark.parametrize("Mo,No", T.SHAPES)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gemm_tn_elementwise(lib, kernel, Mo, No):
    tile, flags = KERNELS[kernel]
    worst, at = 0.0, None
    with forced(lib, flags):
        assert hip.get_option("gemm_flags") == flags
        for K, S, lay in T.CASES:
            for fam in T.FAMILIES:
                xb, xv, ldx, yb, yv, ldy, want, absacc = case(fam, Mo, No, K, lay)
                got = run(lib, tile, xv, ldx, yv, ldy, Mo, No, K, S)
                again = run(lib, tile, xv, ldx, yv, ldy, Mo, No, K, S)
                where = (kernel, Mo, No, K, S, lay, fam)
                assert bool(torch.isfinite(got).all()), where          # a NaN: something outside a window was read
                assert torch.equal(got, again), where
                if fam == "exact":
                    assert torch.equal(got, want.float()), where
                else:
                    r = T.worst_ratio(got, want, T.bound(absacc, K, S))
                    if r > worst:
                        worst, at = r, where
                    assert r <= 1.0, (where, r)
    assert hip.get_option("gemm_flags") == 321
    print(f"gemm_tn {kernel} ({Mo}, {No}): worst |out - want64| / bound {worst:.4f} at K {at[3]} splits {at[4]} layout {at[5]}")


def test_the_entry_refuses_what_the_kernels_cannot_serve(lib):
    Mo, No, K = 16, 24, 40
    X = torch.zeros(K + 1, Mo + 8, dtype=torch.bfloat16, device=DEV)
    Y = torch.zeros(K + 1, No + 8, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(Mo + 1, No + 8, device=DEV)
    ws = torch.zeros(512 + 4 * Mo * No * 4, dtype=torch.uint8, device=DEV)
    x, y, o, w = X.data_ptr(), Y.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert x % 16 == 0 and y % 16 == 0 and o % 16 == 0 and w % 256 == 0
    big = ws.numel() - 256

    def rc(X=x, ldx=Mo, Y=y, ldy=No, out=o, ldo=No, Mo=Mo, No=No, K=K, S=1, tile=128, ws=w, size=big):
        return lib.ditto_gemm_tn_bf16(X, ldx, Y, ldy, out, ldo, Mo, No, K, S, tile, ws, size, stream())

    assert rc() == hip.OK and rc(S=4, tile=256) == hip.OK and rc(ldx=Mo + 8, ldy=No + 8, ldo=No + 8) == hip.OK
    # the four refusals the kernels' 16-byte moves need
    assert rc(ldx=Mo - 8) == hip.ERR_ARG
    assert rc(ldy=No - 8) == hip.ERR_ARG
    assert rc(X=x + 2) == hip.ERR_ARG and rc(X=x + 8) == hip.ERR_ARG
    assert rc(Y=y + 2) == hip.ERR_ARG and rc(Y=y + 8) == hip.ERR_ARG
    assert rc(out=o + 4, S=2) == hip.ERR_ARG and rc(out=o + 8, S=2) == hip.ERR_ARG
    assert rc(out=o + 4, ldo=No + 8) == hip.OK                     # without splits the stores are single words
    # and those it had
    assert rc(tile=64) == hip.ERR_ARG
    assert rc(Mo=Mo + 4, ldx=Mo + 8) == hip.ERR_ARG and rc(No=No + 4, ldy=No + 8, ldo=No + 8) == hip.ERR_ARG
    assert rc(ldx=Mo + 4) == hip.ERR_ARG and rc(ldy=No + 4) == hip.ERR_ARG
    assert rc(ldo=No - 8) == hip.ERR_ARG
    assert rc(ws=w + 128) == hip.ERR_ARG
    assert rc(size=255) == hip.ERR_SIZE
    assert rc(S=4, size=256 + 4 * Mo * No * 4 - 1) == hip.ERR_SIZE and rc(S=4, size=256 + 4 * Mo * No * 4) == hip.OK
    assert rc(S=2, ldo=No + 8) == hip.ERR_ARG
    assert rc(K=0) == hip.ERR_ARG and rc(Mo=0) == hip.ERR_ARG
    torch.cuda.synchronize()
