"""csrc/gemm_frd.hip's bf16-stream form (the one the model's full-row class runs): the residual tile reaches the accumulators
through the LDS (LDS-DMA in whole 128-byte lines, read back in the accumulator layout).  Through ditto_gemm_ln_bf16 with the
"fr_hb" test hook (residual and out bf16).

The accumulators must start from exactly the fp32 values bias + residual, so h is the ONE bf16 rounding of the fp32 h that the
64-row kernel (csrc/gemm_fr64.hip, fp32 stream; pinned bit-equal to this kernel's fp32 form by test_gpu_kernels.py) computes from
the same — bf16-representable — residual: compared bit for bit.  The residual is a hash of (row, column), distinct per element,
so a row or column permutation in the staging path cannot pass; M % 128 in {0, 1, 33, 64, 127} walks the clamp path, whose
redundant rows go through the LDS too."""
import math

import pytest
import torch

import gemm_fr_ref as R
from ditto_tts_amd import hip
from gpu_util import asym, bf16, max_abs, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 768


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip.lib()


def hashed_residual(M):
    """bf16 values from a hash of the element's (row, column): sign, one of seven binades in [2^-5, 4) and seven mantissa bits,
    1 792 different values, every one exact in bf16 (built from its bit pattern)"""
    return R.hashed_residual(M, N).to(torch.bfloat16).contiguous().to(DEV)


def run(lib, tile, hbf, A, Wp, bias, res, out, g, b, u, M, K):
    hip.check(lib.ditto_set_option(b"fr_tile", tile))
    hip.check(lib.ditto_set_option(b"fr_hb", int(hbf)))
    hip.check(lib.ditto_gemm_ln_bf16(A.data_ptr(), K, Wp.data_ptr(), bias.data_ptr(), res.data_ptr(), out.data_ptr(), N,
                                     g.data_ptr() if u is not None else None, b.data_ptr() if u is not None else None,
                                     u.data_ptr() if u is not None else None, N, M, N, K, stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("rot", [0, 3])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("Mrem", [0, 1, 33, 64, 127])
@pytest.mark.parametrize("K", [768, 3072])
def test_bf16_stream_residual_through_lds_is_bitwise_the_64_row_kernels(lib, K, Mrem, inplace, rot):
    M = 128 * (5 if K == 768 else 3) + Mrem
    A = bf16(asym((M, K), 51).to(DEV))
    W = bf16((asym((N, K), 52) / math.sqrt(K)).to(DEV))
    Wp = W.view(N, K // 16, 16).permute(1, 0, 2).contiguous()
    bias = (0.1 * asym((N,), 53)).to(DEV)
    g = (1 + 0.1 * asym((N,), 54)).to(DEV)
    b = (0.1 * asym((N,), 55)).to(DEV)
    r16 = hashed_residual(M)
    assert len(torch.unique(r16[:128].view(torch.int16))) > 1500      # not constants: thousands of different values per tile
    try:
        hip.check(lib.ditto_set_option(b"fr_rot", rot))
        # the fp32 stream on 64-row tiles from the same residual values
        h32 = r16.float().clone()
        u32 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        run(lib, 64, False, A, Wp, bias, h32, h32, g, b, u32, M, K)
        runs = []
        for rep in range(2):
            res = r16.clone()
            out = res if inplace else torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            u = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            run(lib, 130, True, A, Wp, bias, res, out, g, b, u, M, K)
            if not inplace:
                assert torch.equal(res.view(torch.int16), r16.view(torch.int16))           # the residual is only read
            runs.append((out, u))
    finally:
        hip.check(lib.ditto_set_option(b"fr_hb", 0))
        hip.check(lib.ditto_set_option(b"fr_tile", 0))
        hip.check(lib.ditto_set_option(b"fr_rot", 1))
    (h, u), (h2, u2) = runs
    # run to run
    assert torch.equal(h.view(torch.int16), h2.view(torch.int16)) and torch.equal(u.view(torch.int16), u2.view(torch.int16))
    # bit for bit the rounding of the 64-row kernel's fp32 h
    want16 = h32.to(torch.bfloat16)
    bad = (h.view(torch.int16) != want16.view(torch.int16))
    print(f"K {K} M {M} inplace {inplace} rot {rot}: h elements differing from bf16(h of the 64-row kernel): {int(bad.sum())}")
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())
    # backstop against a shared bug: fp64 from the same operands.  fp32 accumulation over K terms of magnitude <= ~1 leaves
    # <= K * 2^-24 * |sum of magnitudes| ~ 1e-4 here; one bf16 rounding of |h| < 16 adds half an ulp = 2^-5 at most.
    want = A.double() @ W.double().T + bias.double() + r16.double()
    err = max_abs(h.double(), want)
    print(f"    max |h - fp64| {err:.3e}")
    assert float(want.abs().max()) < 16 and err <= 2.0 ** -5 + 1e-3
    # u = LayerNorm of the UNROUNDED fp32 row: against fp64 LayerNorm; bf16 output of |y| < 8: half an ulp 2^-6, + 2e-3 for the fp32 statistics
    wu = torch.nn.functional.layer_norm(want, (N,), g.double(), b.double(), 1e-5)
    erru = max_abs(u.double(), wu)
    print(f"    max |u - fp64| {erru:.3e}")
    assert float(wu.abs().max()) < 8 and erru <= 2.0 ** -6 + 2e-3
    assert float((u != u32).float().mean()) < 1e-3      # the 64-row kernel's u: a rounding tie apart (statistics summed per quarter row)


def test_bf16_stream_rejects_a_residual_the_dma_cannot_address(lib):
    """16-byte pieces: an odd leading dimension (in units of 8 elements) or a residual pointer off a 16-byte boundary is an error, not a fault"""
    M, K = 256, 64
    A = bf16(asym((M, K), 61).to(DEV))
    Wp = bf16(asym((N, K), 62).to(DEV)).view(N, K // 16, 16).permute(1, 0, 2).contiguous()
    bias = torch.zeros(N, device=DEV)
    buf = torch.zeros(M * N + 8, dtype=torch.bfloat16, device=DEV)
    try:
        hip.check(lib.ditto_set_option(b"fr_tile", 130))
        hip.check(lib.ditto_set_option(b"fr_hb", 1))
        rc = lib.ditto_gemm_ln_bf16(A.data_ptr(), K, Wp.data_ptr(), bias.data_ptr(), buf.data_ptr() + 8, buf.data_ptr() + 8, N, None, None,
                                    None, N, M, N, K, stream())
        assert rc != hip.OK
        torch.cuda.synchronize()
    finally:
        hip.check(lib.ditto_set_option(b"fr_hb", 0))
        hip.check(lib.ditto_set_option(b"fr_tile", 0))
