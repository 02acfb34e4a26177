"""The guidance-rescale kernels compiled for gfx950 (csrc/guided_rescale.hip), from the compiler's resource report and its listing:
one partial and one finish kernel, neither with scratch memory, and every global load of the partial kernel a 16-byte one — the
offsets, the partner, the prompt length, phi and w come in through scalar loads.  No occupancy is pinned: the four fp64 accumulators
per lane cost registers."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _compile, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
PARTIAL, FINISH = "_ZN5ditto31guidance_rescale_partial_kernel", "_ZN5ditto30guidance_rescale_finish_kernel"


@pytest.fixture(scope="module")
def rescale(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("rescale"), "guided_rescale")


def test_two_kernels_no_scratch(rescale):
    _, remarks = rescale
    partial, finish = _remarks(remarks, PARTIAL), _remarks(remarks, FINISH)
    assert (len(partial), len(finish)) == (1, 1), remarks
    assert {v[0] for v in (*partial.values(), *finish.values())} == {0}, (partial, finish)


def test_partial_kernel_loads_sixteen_bytes_only(rescale):
    asm, _ = rescale
    bodies = _bodies(asm, PARTIAL)
    assert len(bodies) == 1, list(bodies)
    body = next(iter(bodies.values()))
    loads = re.findall(r"global_load_(\w+)", body)
    stores = re.findall(r"global_store_(\w+)", body)
    assert set(loads) == {"dwordx4"}, loads
    assert loads.count("dwordx4") >= 8 + 2, loads               # a whole chunk's round of 4 c + 4 u in flight, and the last chunk's pair
    assert set(stores) == {"dwordx4"} and len(stores) == 2, stores   # the four doubles of a partial
    assert "scratch_" not in body and "buffer_store" not in body and "global_atomic" not in body
