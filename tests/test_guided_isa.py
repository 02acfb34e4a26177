"""The fused guided update (csrc/guided.hip) compiled for gfx950: every instantiation (3 noise sources x with / without CFG) has no
scratch, moves its data with 16-byte global loads and stores only, and keeps full occupancy (8 waves per SIMD)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("guided") / "guided.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ditto_tts_amd", "csrc"), "-w", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(ROOT, "ditto_tts_amd", "csrc", "guided.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return open(out).read(), r.stderr


def _bodies(asm):
    """kernel name -> its instruction text"""
    out = {}
    for m in re.finditer(r"^(_ZN5ditto20guided_update_kernel\w+):.*?$(.*?)^\s*s_endpgm", asm, re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


def test_six_instantiations_no_scratch_full_occupancy(compiled):
    _, remarks = compiled
    names = re.findall(r"Function Name: (_ZN5ditto20guided_update_kernel\S+)", remarks)
    assert len(names) == 6, remarks
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks) == ["0"] * 6, remarks
    assert re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", remarks) == ["8"] * 6, remarks


def test_sixteen_byte_global_accesses_only(compiled):
    asm, _ = compiled
    bodies = _bodies(asm)
    assert len(bodies) == 6, list(bodies)
    for name, body in bodies.items():
        cfg = "Lb1E" in name
        noise_buf = "ILi1E" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        # x, c (+ u under CFG) (+ the noise buffer); one store (+ the unconditional half under CFG)
        assert loads.count("dwordx4") >= 2 + cfg + noise_buf, (name, loads)
        assert stores.count("dwordx4") >= 1 + cfg, (name, stores)
        assert set(stores) == {"dwordx4"}, (name, stores)
        assert set(loads) == {"dwordx4"}, (name, loads)      # the per-utterance scalars (length, a, ce, cz, w, seed): s_load
        assert "scratch_" not in body and "buffer_store" not in body, name
