"""The speech-prompt kernels compiled for gfx950 (csrc/guided_packed.hip: the update behind a prompt is the packed update kernel;
csrc/span_train.hip): the instantiation counts, no scratch, full occupancy (8 waves per SIMD) for the update kernel, and every global
access of the update and noising kernels a 16-byte one — the per-utterance scalars, the prompt length among them, come in through
scalar loads.  Also the home of the helpers the other *_isa tests compile and read listings with."""
import functools
import os
import pathlib
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _compile(tmp, name):
    out = str(tmp / (name + ".s"))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ditto_tts_amd", "csrc"), "-w", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(ROOT, "ditto_tts_amd", "csrc", name + ".hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return open(out).read(), r.stderr


@functools.lru_cache(maxsize=None)
def _listing(name):
    """_compile, once per source file and session"""
    with tempfile.TemporaryDirectory() as tmp:
        return _compile(pathlib.Path(tmp), name)


def _bodies(asm, prefix):
    """kernel name -> its instruction text"""
    return {m.group(1): m.group(2) for m in re.finditer(r"^(%s\w+):.*?$(.*?)^\s*s_endpgm" % prefix, asm, re.M | re.S)}


def _remarks(remarks, prefix):
    """kernel name -> (scratch bytes per lane, waves per SIMD) from the resource-usage remarks"""
    out = {}
    for m in re.finditer(r"Function Name: (%s\S*)(.*?)LDS Size" % prefix, remarks, re.S):
        out[m.group(1)] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", m.group(2)).group(1)),
                           int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", m.group(2)).group(1)))
    return out


UPDATE = "_ZN5ditto27guided_update_packed_kernel"


@pytest.fixture(scope="module")
def prompt():
    return _listing("guided_packed")


@pytest.fixture(scope="module")
def span():
    return _listing("span_train")


def test_update_kernel_twelve_instantiations_no_scratch_full_occupancy(prompt):
    _, remarks = prompt
    res = _remarks(remarks, UPDATE)
    assert len(res) == 12, remarks                               # 3 noise modes x CFG on / off x scalar tag / per-utterance tags
    assert set(res.values()) == {(0, 8)}, res


def test_update_kernel_sixteen_byte_global_accesses_only(prompt):
    asm, _ = prompt
    bodies = _bodies(asm, UPDATE)
    assert len(bodies) == 12, list(bodies)
    for name, body in bodies.items():
        cfg = "ELb1ELb" in name
        noise_buf = "ILi1E" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        assert loads.count("dwordx4") >= 2 + cfg + noise_buf, (name, loads)
        assert stores.count("dwordx4") >= 1 + cfg, (name, stores)


def test_span_kernels_instantiations_no_scratch_and_noise_kernel_accesses(span):
    asm, remarks = span
    noise = _remarks(remarks, "_ZN5ditto24span_noise_packed_kernel")
    mse = _remarks(remarks, "_ZN5ditto22span_mse_packed_kernel")
    fin = _remarks(remarks, "_ZN5ditto22span_mse_finish_kernel")
    assert (len(noise), len(mse), len(fin)) == (2, 2, 1), remarks     # buffer / seeded each, and the ordered sum
    assert {v[0] for v in (*noise.values(), *mse.values(), *fin.values())} == {0}
    bodies = _bodies(asm, "_ZN5ditto24span_noise_packed_kernel")
    assert len(bodies) == 2
    for name, body in bodies.items():
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        assert len(loads) >= 1 + ("ILb0E" in name)                # x0 (+ the noise buffer)
