"""The packed instantiations on the CPU (hipcc only).  attn64q / attn64p of csrc/attention_packed.hip under the checks
tests/test_varlen_isa.py applies to the VARLEN ones (tools/check_attn_loop.py --packed): no scratch and no compiler `s_waitcnt vmcnt`
inside any tile loop, >= 12 wait states between every MFMA write and an asm pair step's read of it, <= 256 VGPRs (2 waves per SIMD).
And the other packed kernels — the guided update, the AdaLN entry, the row map, the text pool, the QKV + RoPE epilogue's GEMMs —
use no scratch (the flat-K 256 x 256 QKV kernel: no more than the dense QKV instantiation it mirrors)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
CSRC = os.path.join(ROOT, "ditto_tts_amd", "csrc")


def _asm(src, extra=()):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, "-w", *extra, "-S", "--cuda-device-only", "-o", "-", os.path.join(CSRC, src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return {m.group(1): int(m.group(2)) for m in
            re.finditer(r"\.amdhsa_kernel (\S+).*?\.amdhsa_private_segment_fixed_size (\d+)", r.stdout, re.S)}


def test_packed_tile_loops_and_asm_wait_states():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_attn_loop.py"), "--packed"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    loops = re.findall(r"^(\S+)\s+\.LBB\d+_\d+\s+mfma\s+(\d+)\s+scratch (\d+)\s+compiler vmcnt waits (\d+)", r.stdout, re.M)
    assert sum("ELb1EEEv" in n for n, *_ in loops) >= 2 * 3 + 2 * 2, r.stdout     # attn64p packed (3 loop blocks) + attn64q (2)
    assert all(s == "0" and w == "0" for _, _, s, w in loops), r.stdout
    rows = re.findall(r"asm reads\s+(\d+)\s+of MFMA results\s+(\d+)\s+min wait states (\d+)\s+\(hipcc's own reads (\d+), min (\d+)\)",
                      r.stdout)
    assert len(rows) == 2, r.stdout                       # attn64q packed: plain and residual
    for _, n_mfma, dmin, n_own, own_min in rows:
        assert int(n_mfma) >= 64 and int(dmin) >= 12 and int(n_own) > 0 and int(own_min) >= 12, r.stdout


def test_packed_attention_keeps_two_waves_per_simd():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, "-w", "-fno-honor-nans", "-fno-slp-vectorize", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, "attention_packed.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    occ = re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)
    assert len(occ) == 4 and all(o == "2" for o in occ), r.stderr
    vg = re.findall(r"VGPRs: (\d+)", r.stderr)
    assert vg and all(int(v) <= 256 for v in vg), r.stderr


def test_packed_rowwise_and_update_kernels_use_no_scratch():
    guided = _asm("guided_packed.hip")
    upd = {k: v for k, v in guided.items() if "guided_update_packed_kernel" in k}
    assert len(upd) == 12 and not any(upd.values()), upd                # 3 noise sources x CFG on / off x scalar tag / per-utterance tags
    rw = _asm("rowwise.hip")
    adaln = {k: v for k, v in rw.items() if re.search(r"ln_kernelILi\dELi3EE", k)}
    assert len(adaln) == 8 and not any(adaln.values()), adaln           # every row width of the packed AdaLN entry
    for name in ("packed_row_map_kernel", "text_pool_packed_kernel"):
        ks = [v for k, v in rw.items() if name in k]
        assert ks == [0], (name, ks)


def test_packed_qkv_epilogue_kernels_use_no_scratch():
    g = _asm("gemm.hip")
    packed = {k: v for k, v in g.items() if re.search(r"gemm128(_deep)?_kernelILi9EE", k)}
    assert len(packed) == 2 and not any(packed.values()), packed        # the 128 x 128 kernels
    g256 = _asm("gemm256.hip")
    p256 = {k: v for k, v in g256.items() if "gemm256_kernelILi9E" in k}
    assert len(p256) == 3, p256
    for k, v in p256.items():
        dense = g256[k.replace("ILi9E", "ILi2E")]                        # the dense QKV + RoPE instantiation of the same schedule
        assert v <= dense, (k, v, dense)
        if "ELb1ELb0ELb1EE" not in k:                                     # (the flat-K schedule keeps a few bytes, as the dense one)
            assert v == 0, (k, v)
