"""The multistep update kernel compiled for gfx950 (csrc/guided_multistep.hip), from the compiler's resource report and its listing:
four instantiations (CFG on / off x one step for the batch / one per utterance), no scratch, full occupancy (8 waves per SIMD) like the
other update kernels, and every global access a 16-byte one — the per-utterance block (coefficients, guidance scale, use_prev) and the
offsets and both context lengths come in through scalar loads."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _listing, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
KERNEL = "_ZN5ditto23multistep_update_kernel"


@pytest.fixture(scope="module")
def multistep():
    return _listing("guided_multistep")


def test_four_instantiations_no_scratch_full_occupancy(multistep):
    _, remarks = multistep
    res = _remarks(remarks, KERNEL)
    assert len(res) == 4, remarks
    assert set(res.values()) == {(0, 8)}, res


def test_sixteen_byte_global_accesses_only(multistep):
    asm, _ = multistep
    bodies = _bodies(asm, KERNEL)
    assert len(bodies) == 4, list(bodies)
    for name, body in bodies.items():
        cfg = "ILb1ELb" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        # both bodies (with and without history) are in the kernel: x, c (+ u) each, and q in the one with history
        assert loads.count("dwordx4") >= 2 * (2 + cfg) + 1, (name, loads)
        assert stores.count("dwordx4") >= 2 * (2 + cfg), (name, stores)        # x' (both halves under CFG) and q, in each body
