"""The packed update, multistep and span-training kernels compiled for gfx950 (csrc/guided_packed.hip, csrc/guided_multistep.hip,
csrc/span_train.hip), from the compiler's resource report and its listing: 12 update, 4 multistep and 2 + 2 span instantiations behind
the unprompted, per-utterance-tag, speech-prompt and speech-infilling entries alike, no scratch, full occupancy (8 waves per SIMD),
and every global access of the update and multistep kernels a 16-byte one — the per-utterance scalars, the tag and both context
lengths among them, come in through scalar loads."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _listing, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
UPDATE = "_ZN5ditto27guided_update_packed_kernel"
MULTISTEP = "_ZN5ditto23multistep_update_kernel"
NOISE = "_ZN5ditto24span_noise_packed_kernel"
MSE = "_ZN5ditto22span_mse_packed_kernel"


@pytest.fixture(scope="module")
def update():
    return _listing("guided_packed")


@pytest.fixture(scope="module")
def multistep():
    return _listing("guided_multistep")


@pytest.fixture(scope="module")
def span():
    return _listing("span_train")


def test_instantiations_no_scratch_full_occupancy(update, multistep, span):
    upd = _remarks(update[1], UPDATE)
    ms = _remarks(multistep[1], MULTISTEP)
    noise = _remarks(span[1], NOISE)
    mse = _remarks(span[1], MSE)
    # update: 3 noise modes x CFG on / off x scalar tag / per-utterance tags; span: buffer / seeded each
    assert (len(upd), len(ms), len(noise), len(mse)) == (12, 4, 2, 2), (update[1], multistep[1], span[1])
    assert sum("Lb1EEEv" in n for n in upd) == 6, list(upd)             # TAGS, the last template argument, true
    for res in (upd, ms, noise, mse):
        assert set(res.values()) == {(0, 8)}, res


def test_update_kernels_sixteen_byte_global_accesses_only(update, multistep):
    asm, _ = update
    bodies = _bodies(asm, UPDATE)
    assert len(bodies) == 12, list(bodies)
    for name, body in bodies.items():
        cfg = "ELb1ELb" in name
        noise_buf = "ILi1E" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        # x, c (+ u under CFG) (+ the noise buffer); one store (+ the unconditional half under CFG)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        assert loads.count("dwordx4") >= 2 + cfg + noise_buf, (name, loads)
        assert stores.count("dwordx4") >= 1 + cfg, (name, stores)
    bodies = _bodies(multistep[0], MULTISTEP)
    assert len(bodies) == 4, list(bodies)
    for name, body in bodies.items():
        cfg = "ILb1ELb" in name
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        assert loads.count("dwordx4") >= 2 * (2 + cfg) + 1, (name, loads)      # both bodies: x, c (+ u) each, q in the one with history
        assert stores.count("dwordx4") >= 2 * (2 + cfg), (name, stores)        # x' (both halves under CFG) and q, in each body


def test_span_noise_kernel_sixteen_byte_global_accesses_only(span):
    asm, _ = span
    bodies = _bodies(asm, NOISE)
    assert len(bodies) == 2
    for name, body in bodies.items():
        loads = re.findall(r"global_load_(\w+)", body)
        stores = re.findall(r"global_store_(\w+)", body)
        assert set(loads) == {"dwordx4"} and set(stores) == {"dwordx4"}, (name, loads, stores)
        assert len(loads) >= 1 + ("ILb0E" in name)                # x0 (+ the noise buffer)
