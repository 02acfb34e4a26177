"""The kernels of projected guidance over a request stream's mixed layout compiled for gfx950 (csrc/guided_project_mixed.hip), from the
compiler's resource report and its listing, as tests/test_refresh_isa.py reads them: launch 1, the finish and the three instantiations
of the update (the noise modes) use no scratch, and every global access is a 16-byte one — kind[b], partner[b], the offsets, the
prompt length, proj[b] and the coefficients come in through scalar loads."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _listing, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
# prefix -> instantiations
KERNELS = {"_ZN5ditto37guidance_project_partial_mixed_kernel": 1, "_ZN5ditto36guidance_project_finish_mixed_kernel": 1,
           "_ZN5ditto34guided_update_project_mixed_kernel": 3}


@pytest.fixture(scope="module")
def mixed():
    return _listing("guided_project_mixed")


def test_every_instantiation_without_scratch(mixed):
    asm, remarks = mixed
    for prefix, count in KERNELS.items():
        res = _remarks(remarks, prefix)
        assert len(res) == count, (prefix, remarks)
        assert {scratch for scratch, _ in res.values()} == {0}, res                 # private segment size 0
        for name in res:
            desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, re.S)
            assert desc and re.search(r"\.amdhsa_private_segment_fixed_size 0\n", desc.group(1)), name


def test_sixteen_byte_global_accesses_only(mixed):
    asm, _ = mixed
    for prefix, count in KERNELS.items():
        bodies = _bodies(asm, prefix)
        assert len(bodies) == count, (prefix, list(bodies))
        for name, body in bodies.items():
            loads = re.findall(r"global_load_(\w+)", body)
            stores = re.findall(r"global_store_(\w+)", body)
            assert loads and stores, name
            assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
