"""The mixed-step update kernel compiled for gfx950 (csrc/guided_mixed.hip), from the compiler's resource report and its listing: three
instantiations (the noise modes), no scratch, full occupancy (8 waves per SIMD) like the other update kernels, and every global
access a 16-byte one — partner[b], the offsets, the prompt length and the coefficients come in through scalar loads."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _compile, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
KERNEL = "_ZN5ditto26guided_update_mixed_kernel"


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("mixed"), "guided_mixed")


def test_three_instantiations_no_scratch_full_occupancy(mixed):
    _, remarks = mixed
    res = _remarks(remarks, KERNEL)
    assert len(res) == 3, remarks
    assert set(res.values()) == {(0, 8)}, res


def test_sixteen_byte_global_accesses_only(mixed):
    asm, _ = mixed
    bodies = _bodies(asm, KERNEL)
    assert len(bodies) == 3, list(bodies)
    for name, body in bodies.items():
        noise_buf = "ILi1E" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        # both bodies are in the kernel: guided x, c, u (+ the noise buffer) read and two copies written; unguided x, c (+ noise), one
        assert loads.count("dwordx4") >= (3 + noise_buf) + (2 + noise_buf), (name, loads)
        assert stores.count("dwordx4") >= 2 + 1, (name, stores)
        assert "scratch_" not in body and "buffer_store" not in body, name
