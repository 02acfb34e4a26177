"""The VARLEN instantiations of attn64q / attn64p (csrc/attention_varlen.hip) under the checks tests/test_kernel_isa.py applies to the
dense ones (tools/check_attn_loop.py --varlen): no scratch and no compiler `s_waitcnt vmcnt` inside any tile loop, >= 12 wait states
between every MFMA write and an asm pair step's read of it; and the dense kernels' occupancy (<= 256 VGPRs: 2 waves per SIMD)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def test_varlen_tile_loops_and_asm_wait_states():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_attn_loop.py"), "--varlen"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    loops = re.findall(r"^(\S+)\s+\.LBB\d+_\d+\s+mfma\s+(\d+)\s+scratch (\d+)\s+compiler vmcnt waits (\d+)", r.stdout, re.M)
    assert sum("ELb1EEEv" in n for n, *_ in loops) >= 2 * 3 + 2 * 2, r.stdout     # attn64p VARLEN (3 loop blocks) + attn64q VARLEN (2)
    assert all(s == "0" and w == "0" for _, _, s, w in loops), r.stdout
    rows = re.findall(r"asm reads\s+(\d+)\s+of MFMA results\s+(\d+)\s+min wait states (\d+)\s+\(hipcc's own reads (\d+), min (\d+)\)",
                      r.stdout)
    assert len(rows) == 2, r.stdout                       # attn64q VARLEN: plain and residual
    for _, n_mfma, dmin, n_own, own_min in rows:
        assert int(n_mfma) >= 64 and int(dmin) >= 12 and int(n_own) > 0 and int(own_min) >= 12, r.stdout


def test_varlen_kernels_keep_two_waves_per_simd():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ditto_tts_amd", "csrc"), "-w", "-fno-honor-nans", "-fno-slp-vectorize", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
                        os.path.join(ROOT, "ditto_tts_amd", "csrc", "attention_varlen.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    occ = re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)
    assert len(occ) == 4 and all(o == "2" for o in occ), r.stderr
