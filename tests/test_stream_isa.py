"""The kernels of continuous batching compiled for gfx950 (csrc/guided_packed.hip: the per-utterance-tag update is the TAGS half of
the packed update kernel's instantiations; csrc/regroup_packed.hip): no scratch, full occupancy (8 waves per SIMD), and every global
access a 16-byte one — the per-utterance scalars, the tag among them, and the segment of a regroup come in through scalar loads."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_prompt_isa import _listing, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _compile(tmp, name):
    out = str(tmp / (name + ".s"))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ditto_tts_amd", "csrc"), "-w", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(ROOT, "ditto_tts_amd", "csrc", name + ".hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return open(out).read(), r.stderr


def _bodies(asm, prefix):
    """kernel name -> its instruction text"""
    return {m.group(1): m.group(2) for m in re.finditer(r"^(%s\w+):.*?$(.*?)^\s*s_endpgm" % prefix, asm, re.M | re.S)}


UPDATE = "_ZN5ditto27guided_update_packed_kernel"


@pytest.fixture(scope="module")
def tags():
    return _listing("guided_packed")


@pytest.fixture(scope="module")
def regroup(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("regroup"), "regroup_packed")


def test_tag_kernel_six_instantiations_no_scratch_full_occupancy(tags):
    _, remarks = tags
    res = _remarks(remarks, UPDATE)
    assert len(res) == 12 and sum("Lb1EEEv" in n for n in res) == 6, remarks      # TAGS, the last template argument: six of the twelve
    assert set(res.values()) == {(0, 8)}, res


def test_tag_kernel_sixteen_byte_global_accesses_only(tags):
    asm, _ = tags
    bodies = _bodies(asm, UPDATE)
    assert len(bodies) == 12 and sum("Lb1EEEv" in n for n in bodies) == 6, list(bodies)
    for name, body in bodies.items():
        cfg = "ELb1ELb" in name
        noise_buf = "ILi1E" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        # x, c (+ u under CFG) (+ the noise buffer); one store (+ the unconditional half under CFG)
        assert loads.count("dwordx4") >= 2 + cfg + noise_buf, (name, loads)
        assert stores.count("dwordx4") >= 1 + cfg, (name, stores)
        assert set(stores) == {"dwordx4"}, (name, stores)
        assert set(loads) == {"dwordx4"}, (name, loads)      # offsets, a, ce, cz, w, seed and the TAG: s_load
        assert "scratch_" not in body and "buffer_store" not in body, name
        assert "s_load" in body, name


def test_regroup_kernel_no_scratch_sixteen_byte_copies(regroup):
    asm, remarks = regroup
    names = re.findall(r"Function Name: (_ZN5ditto21regroup_packed_kernel\S+)", remarks)
    assert len(names) == 1, remarks
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks) == ["0"], remarks
    assert re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", remarks) == ["8"], remarks
    (body,) = _bodies(asm, "_ZN5ditto21regroup_packed_kernel").values()
    loads = re.findall(r"global_load_(\w+)", body)
    stores = re.findall(r"global_store_(\w+)", body)
    assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (loads, stores)
    assert loads.count("dwordx4") >= 5                        # four in flight in the main loop, one in the tail
    assert "scratch_" not in body and "buffer_store" not in body
