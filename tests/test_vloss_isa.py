"""The v objective's span-loss kernel compiled for gfx950 (csrc/span_train.hip span_vloss_packed_kernel), from the compiler's resource
report and its listing: two instantiations (a noise buffer, seeds), no scratch, full occupancy (8 waves per SIMD) like its MSE sibling,
every streamed access a 16-byte one — pred, x0 (and the noise buffer) in, the gradient out; the one 4-byte store is the workgroup's
partial sum — and no atomics."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _listing, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
VLOSS = "_ZN5ditto24span_vloss_packed_kernel"


@pytest.fixture(scope="module")
def span():
    return _listing("span_train")


def test_two_instantiations_no_scratch_full_occupancy(span):
    res = _remarks(span[1], VLOSS)
    assert len(res) == 2, span[1]
    assert set(res.values()) == {(0, 8)}, res


def test_streams_move_in_sixteen_byte_accesses_and_nothing_is_atomic(span):
    bodies = _bodies(span[0], VLOSS)
    assert len(bodies) == 2, list(bodies)
    for name, body in bodies.items():
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"}, (name, loads)
        assert len(loads) >= 2 + ("ILb0E" in name), (name, loads)          # pred, x0 (+ the noise buffer)
        assert set(stores) == {"dwordx4", "dword"} and stores.count("dword") == 1, (name, stores)
        assert "atomic" not in body, name
