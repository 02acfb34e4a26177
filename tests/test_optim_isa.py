"""The fused optimizer's kernels compiled for gfx950 (csrc/optim.hip), from the compiler's resource report and its listing: four
kernels, none with scratch memory, no global atomics; every vector load of the norm-partial kernel a 16-byte one (the table comes in
through scalar loads); every vector load of the apply and swap kernels a 16-byte one, their bulk stores 16-byte ones beside the single
dwords of a segment's last 1 - 3 elements (and, in the apply kernel, the state's next slot).  No occupancy is pinned."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _compile, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
PARTIAL, FINISH = "_ZN5ditto27optim_sqnorm_partial_kernel", "_ZN5ditto24optim_norm_finish_kernel"
APPLY, SWAP = "_ZN5ditto24optim_adamw_apply_kernel", "_ZN5ditto17optim_swap_kernel"


@pytest.fixture(scope="module")
def optim(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("optim"), "optim")


def _one(asm, prefix):
    bodies = _bodies(asm, prefix)
    assert len(bodies) == 1, list(bodies)
    return next(iter(bodies.values()))


def test_four_kernels_no_scratch(optim):
    _, remarks = optim
    res = [_remarks(remarks, k) for k in (PARTIAL, FINISH, APPLY, SWAP)]
    assert [len(r) for r in res] == [1, 1, 1, 1], remarks
    assert {v[0] for r in res for v in r.values()} == {0}, res


def test_no_global_atomics_no_flat_or_scratch_accesses(optim):
    asm, _ = optim
    for k in (PARTIAL, FINISH, APPLY, SWAP):
        body = _one(asm, k)
        assert "global_atomic" not in body and "flat_" not in body and "scratch_" not in body and "buffer_" not in body, k


def test_partial_kernel_loads_sixteen_bytes_only(optim):
    asm, _ = optim
    body = _one(asm, PARTIAL)
    loads = re.findall(r"global_load_(\w+)", body)
    stores = re.findall(r"global_store_(\w+)", body)
    assert set(loads) == {"dwordx4"}, loads
    assert len(loads) >= 4 + 1, loads                           # a whole chunk's round of 4 in flight, and the last chunk's one
    assert stores == ["dwordx2"], stores                        # the chunk's double


def test_apply_and_swap_kernels_move_sixteen_bytes(optim):
    asm, _ = optim
    body = _one(asm, APPLY)
    loads = re.findall(r"global_load_(\w+)", body)
    stores = re.findall(r"global_store_(\w+)", body)
    assert set(loads) == {"dwordx4"}, loads                     # the state and the table are scalar loads
    assert len(loads) >= (20 + 5) + (16 + 4), loads             # with / without an average: a round of 4 quads of 5 / 4 arrays, + the tail's
    assert set(stores) <= {"dwordx4", "dword", "dwordx2"}, stores   # (dwordx2: clip and skip beside the next slot)
    assert stores.count("dwordx4") >= 16 + 12 + 4 + 3, stores
    assert "ds_" not in body                                    # no LDS
    body = _one(asm, SWAP)
    loads = re.findall(r"global_load_(\w+)", body)
    stores = re.findall(r"global_store_(\w+)", body)
    assert set(loads) == {"dwordx4"} and len(loads) >= 8 + 2, loads
    assert set(stores) == {"dwordx4", "dword"} and stores.count("dwordx4") >= 8 + 2, stores
