"""The three-kind update kernel of a refresh stream compiled for gfx950 (csrc/guided_refresh.hip), from the compiler's resource report
and its listing: three instantiations (the noise modes), no scratch, and every global access a 16-byte one — kind[b], partner[b], the
offsets, the prompt length and the coefficients come in through scalar loads, as tests/test_mixed_isa.py checks for the mixed kernel."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _listing, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
KERNEL = "_ZN5ditto28guided_update_refresh_kernel"


@pytest.fixture(scope="module")
def refresh():
    return _listing("guided_refresh")


def test_three_instantiations_no_scratch(refresh):
    _, remarks = refresh
    res = _remarks(remarks, KERNEL)
    assert len(res) == 3, remarks
    assert {scratch for scratch, _ in res.values()} == {0}, res                 # private segment size 0


def test_sixteen_byte_global_accesses_only(refresh):
    asm, _ = refresh
    bodies = _bodies(asm, KERNEL)
    assert len(bodies) == 3, list(bodies)
    for name, body in bodies.items():
        noise_buf = "ILi1E" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        # the three bodies are in the kernel: refresh x, c, u read and x', the copy, delta written; reuse x, c, delta read and x'
        # written; plain x, c read and x' written (+ the noise buffer each)
        assert loads.count("dwordx4") >= (3 + noise_buf) + (3 + noise_buf) + (2 + noise_buf), (name, loads)
        assert stores.count("dwordx4") >= 3 + 1 + 1, (name, stores)
        assert "scratch_" not in body and "buffer_store" not in body, name
        desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, re.S)
        assert desc and re.search(r"\.amdhsa_private_segment_fixed_size 0\n", desc.group(1)), name
