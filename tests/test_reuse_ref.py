"""The DERIVED bound of the guidance-reuse LOAD step (tests/reuse_ref.py) tried on the host, on the inputs the GPU test
(test_gpu_reuse_update.py) uses: it admits an fp32 imitation of the kernels' arithmetic in every noise mode and both multistep
branches, and it refuses each modelled defect by a wide margin."""
import pytest
import torch

import reuse_ref as R


@pytest.fixture(scope="module")
def inp():
    return R.Inputs("small")


def _noise(inp, noise):
    return None if noise == "none" else inp.z if noise == "buffer" else R.philox_window(inp)


@pytest.mark.parametrize("noise", ["philox", "none", "buffer"])
def test_the_bound_admits_an_fp32_imitation_of_the_strided_load(inp, noise):
    want, bound = R.load_fp64(inp, inp.c, inp.delta, inp.x, _noise(inp, noise))
    gen = inp.gen_mask()
    assert float(bound[~gen].max()) == 0 and float(bound[gen].min()) > 0
    got = R.imitate_load(inp, noise)
    assert torch.equal(got[~gen], inp.x[~gen])                                   # the imitation leaves the context rows alone
    ratio = R.worst_ratio(torch.where(gen[:, None], got, torch.zeros(())), want, bound)
    print(f"strided load, {noise}: worst admitted ratio {ratio:.3f}")
    assert 0 < ratio <= 1.0


@pytest.mark.parametrize("use_prev", [False, True], ids=["first_step", "use_prev"])
def test_the_bound_admits_an_fp32_imitation_of_the_multistep_load(inp, use_prev):
    want, bound, want_q, bound_q = R.multistep_load_fp64(inp, inp.c, inp.delta, inp.x, inp.q, use_prev)
    gen = inp.gen_mask()
    got, got_q = R.imitate_load(inp, "none", multistep=True, use_prev=use_prev)
    g2, zero = gen[:, None], torch.zeros(())
    r_x = R.worst_ratio(torch.where(g2, got, zero), want, bound)
    r_q = R.worst_ratio(torch.where(g2, got_q, zero), want_q, bound_q)
    print(f"multistep load, use_prev {use_prev}: worst admitted ratio x' {r_x:.3f}, q' {r_q:.3f}")
    assert 0 < r_x <= 1.0 and 0 < r_q <= 1.0


def test_w_equal_one_makes_the_load_the_unguided_update(inp):
    """e = fma(0, delta, c) = c exactly: what the GPU test pins the draw and the coefficient plumbing with"""
    keep = inp.w.clone()
    inp.w[:] = 1.0
    try:
        got = R.imitate_load(inp, "buffer")
        other = R.imitate_load(inp, "buffer", bug="delta_sign")                  # delta does not matter at all
    finally:
        inp.w[:] = keep
    assert torch.equal(got, other)


@pytest.mark.parametrize("bug", ["w_not_wm1", "delta_sign", "delta_global", "global_philox", "delta_uncond"])
def test_the_strided_bound_refuses_each_modelled_defect(inp, bug):
    noise = "philox" if bug == "global_philox" else "buffer"
    want, bound = R.load_fp64(inp, inp.c, inp.delta, inp.x, _noise(inp, noise))
    got = R.imitate_load(inp, noise, bug=bug)
    ratio = R.worst_ratio(torch.where(inp.gen_mask()[:, None], got, torch.zeros(())), want, bound)
    print(f"strided load, {bug}: least refused ratio {ratio:.3e}")
    assert ratio > 100.0


@pytest.mark.parametrize("bug", ["w_not_wm1", "delta_sign", "delta_global", "delta_uncond", "no_kx"])
def test_the_multistep_bound_refuses_each_modelled_defect(inp, bug):
    want, bound, want_q, bound_q = R.multistep_load_fp64(inp, inp.c, inp.delta, inp.x, inp.q, True)
    got, got_q = R.imitate_load(inp, "none", multistep=True, use_prev=True, bug=bug)
    g2, zero = inp.gen_mask()[:, None], torch.zeros(())
    r_x = R.worst_ratio(torch.where(g2, got, zero), want, bound)
    r_q = R.worst_ratio(torch.where(g2, got_q, zero), want_q, bound_q)
    print(f"multistep load, {bug}: least refused ratio x' {r_x:.3e}, q' {r_q:.3e}")
    assert r_x > 100.0 and r_q > 100.0
