"""The packed training kernels on the CPU (hipcc only): csrc/attention_train_packed.hip, csrc/attention_bwd_packed.hip and
csrc/train_packed.hip cross-compiled for gfx950.  From the compiler's resource report every packed kernel uses no more scratch than
the dense instantiation it mirrors (0 where that one has 0) and keeps its waves-per-SIMD occupancy — both bounds read from the dense
translation unit compiled in the same test, not written down as numbers."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
CSRC = os.path.join(ROOT, "ditto_tts_amd", "csrc")


def _report(src, extra):
    """{kernel name: (scratch bytes per lane, waves per SIMD, VGPRs)} from -Rpass-analysis=kernel-resource-usage"""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, "-w", *extra, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
                        os.path.join(CSRC, src)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    out = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                         r.stderr, re.S):
        out[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(2)))
    return out


def _key(name, kernel):
    """the template arguments of `kernel` in a mangled name (the part that is the same in the dense and the packed unit)"""
    m = re.search(kernel + r"(I\w+?E)EvN", name)
    assert m, name
    return m.group(1)


def test_packed_training_forward_attention_mirrors_the_dense_instantiations():
    flags = ["-fno-honor-nans", "-fno-slp-vectorize"]
    dense = {_key(k, "attn64v2_kernel"): v for k, v in _report("attention_train.hip", flags).items() if "attn64v2_kernel" in k}
    packed = {_key(k, "attn64v2_kernel"): v for k, v in _report("attention_train_packed.hip", flags).items() if "attn64v2_kernel" in k}
    assert len(dense) == 4 and sorted(packed) == sorted(dense), (dense, packed)     # <RESID> x <DROP>, TRAIN, 3 waves per SIMD
    for k, (scratch, occ, _) in packed.items():
        assert scratch <= dense[k][0] and occ == dense[k][1], (k, packed[k], dense[k])


def test_packed_attention_backward_mirrors_the_dense_instantiations():
    flags = ["-fno-slp-vectorize"]
    dense = {_key(k, "attn64_bwd_kernel"): v for k, v in _report("attention_bwd.hip", flags).items() if "attn64_bwd_kernel" in k}
    packed = {_key(k, "attn64_bwd_kernel"): v for k, v in _report("attention_bwd_packed.hip", flags).items() if "attn64_bwd_kernel" in k}
    assert len(dense) == 6 and len(packed) == 4, (dense, packed)     # packed: dq always with the key mask (x DROP), dk,dv (x DROP)
    for k, (scratch, occ, _) in packed.items():
        assert k in dense, k
        assert scratch <= dense[k][0] and occ == dense[k][1], (k, packed[k], dense[k])


def test_per_utterance_adaln_backward_uses_no_more_scratch_than_the_grouped_one():
    dense = {k: v for k, v in _report("train.hip", []).items() if re.search(r"ln_bwd_kernelILi\dELb0ELb0ELb0EE", k)}
    packed = _report("train_packed.hip", [])
    seg = {k: v for k, v in packed.items() if "adaln_bwd_packed_kernel" in k}
    assert len(dense) == 8 and len(seg) == 8, (sorted(dense), sorted(seg))           # every row width d / 256
    for k, (scratch, occ, _) in seg.items():
        ch = re.search(r"adaln_bwd_packed_kernelILi(\d)E", k).group(1)
        (ds, docc, _), = [v for n, v in dense.items() if f"ln_bwd_kernelILi{ch}E" in n]
        assert scratch <= ds and occ >= docc, (k, seg[k], (ds, docc))
    fin = [v for k, v in packed.items() if "segment_partials_kernel" in k]
    assert len(fin) == 1 and fin[0][0] == 0, fin
