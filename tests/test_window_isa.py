"""The speech-infilling kernels compiled for gfx950 (csrc/guided_window.hip, csrc/span_window.hip), from the compiler's resource report
and its listing: 12 + 4 update and 2 + 2 span instantiations, no scratch, full occupancy (8 waves per SIMD), and every global access
of the update kernels a 16-byte one — the per-utterance scalars, both context lengths among them, come in through scalar loads."""
import os
import re

import pytest

from test_prompt_isa import _bodies, _compile, _remarks

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
UPDATE = "_ZN5ditto27guided_update_window_kernel"
MULTISTEP = "_ZN5ditto30multistep_update_window_kernel"
NOISE = "_ZN5ditto24span_noise_window_kernel"
MSE = "_ZN5ditto22span_mse_window_kernel"


@pytest.fixture(scope="module")
def window(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("window"), "guided_window")


@pytest.fixture(scope="module")
def span(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("span_window"), "span_window")


def test_instantiations_no_scratch_full_occupancy(window, span):
    upd = _remarks(window[1], UPDATE)
    ms = _remarks(window[1], MULTISTEP)
    noise = _remarks(span[1], NOISE)
    mse = _remarks(span[1], MSE)
    assert (len(upd), len(ms), len(noise), len(mse)) == (12, 4, 2, 2), (window[1], span[1])
    for res in (upd, ms, noise, mse):
        assert set(res.values()) == {(0, 8)}, res


def test_update_kernels_sixteen_byte_global_accesses_only(window):
    asm, _ = window
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
    bodies = _bodies(asm, MULTISTEP)
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
