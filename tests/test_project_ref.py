"""Projected guidance on the host (no GPU): tests/project_ref.py's restatement of the contract of include/ditto_project.h against the
paper's algorithm written out directly, the plain-CFG special case, the exact fp32 fma the GPU test restates the kernels' chains with,
the DERIVED bounds — an fp32 emulation of the kernels summed in another order stays inside them on every one of the GPU test's inputs
(largest ratio measured 0.92) and each modelled defect leaves them on every input it applies to (smallest ratio measured 7e3) — and
the keyword validation and the refusals of the sampling entries, which run before any device work."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import project_ref as R
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import guidance_vector, multistep_schedule, project_table, projection_vectors
from test_interval_host import _bare_generator

CASES = [(name, b) for name in sorted(R.SHAPES) for b in range(4)]
IDS = [f"{n}-{b}" for n, b in CASES]


@pytest.mark.parametrize("name,b", CASES, ids=IDS)
def test_contract_is_the_papers_algorithm(name, b):
    """eps and v coefficients, momentum on and off, threshold off, inactive and active: 1e-12 relative"""
    w, _ = R.window(name, b)
    p = R.case_par(name, b)
    ref = R.reference(*w, p)
    e, m_new = R.apg_direct(*w, p)
    assert np.max(np.abs(e - ref["e"])) <= 1e-12 * np.max(np.abs(ref["e"]))
    assert np.max(np.abs(m_new - ref["m_new"])) <= 1e-12 * np.max(np.abs(ref["m_new"]))
    # and with this window under the other parameter sets too
    for q in R.PARS:
        if q["use_prev"] and not p["use_prev"]:
            continue                                          # this utterance's m is NaN
        ref, (e, _) = R.reference(*w, q), R.apg_direct(*w, q)
        assert np.max(np.abs(e - ref["e"])) <= 1e-12 * np.max(np.abs(ref["e"]))


@pytest.mark.parametrize("coef", [(R.KX_EPS, R.KE_EPS), (R.KX_V, R.KE_V)], ids=["eps", "v"])
def test_eta_one_is_plain_cfg(coef):
    (x, c, u, m), _ = R.window("d256", 2)
    for w in (5.0, 1.0, 0.0, 2.5):
        ref = R.reference(x, c, u, m, R.par(*coef, w, 1.0))
        c64, u64 = c.astype(np.float64).ravel(), u.astype(np.float64).ravel()
        want = u64 + w * (c64 - u64)
        assert ref["fx"] == 0.0 and ref["fc"] == 1.0
        assert np.max(np.abs(ref["e"] - want)) <= 1e-12 * np.max(np.abs(want))


def test_degenerate_cases():
    (x, c, u, m), _ = R.window("d64", 3)
    assert R._finish(1.0, 1.0, 1.0, 4.0, R.par(1.0, 0.0, 5.0, 0.0))[:3] == (0.0, 1.0, 0.0)            # ke == 0
    assert R._finish(1.0, 1.0, 0.0, 4.0, R.par(1.0, -1.0, 5.0, 0.0))[:2] == (0.0, 1.0)                  # S_DD == 0: p = 0
    assert R._finish(1.0, 1.0, float("inf"), 4.0, R.par(1.0, -1.0, 5.0, 0.0))[4] == 0.0
    assert R._finish(float("inf"), 1.0, 1.0, 4.0, R.par(1.0, -1.0, 5.0, 0.0, r=1.0))[3] == 1.0          # rms not finite: rho = 1
    assert R._finish(4.0, 1.0, 1.0, 4.0, R.par(1.0, -1.0, 5.0, 0.0, r=1.0))[3] == 1.0                   # rms == r: not above it
    assert R._finish(16.0, 1.0, 1.0, 4.0, R.par(1.0, -1.0, 5.0, 0.0, r=1.0))[3] == 0.5
    hi, lo = R.par(1.0, -1.0, 5.0, 7.0), R.par(1.0, -1.0, 5.0, -3.0)                                      # eta is clamped into [0, 1]
    assert R._finish(1.0, 1.0, 1.0, 4.0, hi)[:3] == R._finish(1.0, 1.0, 1.0, 4.0, R.par(1.0, -1.0, 5.0, 1.0))[:3]
    assert R._finish(1.0, 1.0, 1.0, 4.0, lo)[:3] == R._finish(1.0, 1.0, 1.0, 4.0, R.par(1.0, -1.0, 5.0, 0.0))[:3]


def test_fma32_is_the_exact_fused_multiply_add():
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(4000).astype(np.float32), rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.standard_normal(4000) * 2.0 ** -20)).astype(np.float32)   # cancelling
    # ties of the double rounding: a * b + c lands an fp32 half-ulp plus a bit the fp64 sum cannot hold
    a = np.concatenate([a, np.float32([1 + 2.0 ** -23, 1 + 2.0 ** -23, 3.0])])
    b = np.concatenate([b, np.float32([1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** -60])])
    c = np.concatenate([c, np.float32([2.0 ** 30, 2.0 ** 29, 1 + 2.0 ** -23])])
    got = R.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                      # Python rounds a Fraction to fp64 correctly; then bracket
        cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))}
        best = min(cands, key=lambda v: (abs(Fraction(v) - exact), int(np.float32(v).view(np.int32)) & 1))
        assert float(got[i]) == best, i


@pytest.mark.parametrize("name,b", CASES, ids=IDS)
def test_emulation_stays_inside_the_bounds(name, b):
    w, _ = R.window(name, b)
    p = R.case_par(name, b)
    f, m_new, e = R.emulate(*w, p)
    assert R.ratio(*w, p, f, m_new, e) <= 1.0
    # the coefficients alone, summed in the kernels' chunks serially, too
    md, Dd = (v.astype(np.float64) for v in R.direction32(*w, p))
    tot = lambda v: float(np.cumsum([float(np.cumsum(v[k:k + 4 * R.CHUNK_QUADS])[-1]) for k in range(0, v.size, 4 * R.CHUNK_QUADS)])[-1])
    f2 = np.array(R._finish(tot(md * md), tot(md * Dd), tot(Dd * Dd), float(md.size), p)[:3], np.float32)
    assert R.ratio(*w, p, f2, m_new, R.e32(w[0], w[1], m_new, f2)) <= 1.0


def _applies(defect, name, b):
    """the inputs on which a defect changes anything: the others compute the same numbers with or without it"""
    p, (_, _, q) = R.case_par(name, b), R.SHAPES[name][1][b]
    statistics_matter = p["eta"] < 1.0 or p["r"] > 0.0
    return {"project_on_u": p["eta"] < 1.0, "norm_not_rms": p["r"] > 0.0 and R.SHAPES[name][1][b][0] * R.SHAPES[name][0] > 1,
            "threshold_into_m": p["r"] > 0.0 and R.reference(*R.window(name, b)[0], p)["rho"] < 1.0,
            "beta_sign": bool(p["use_prev"]) and p["beta"] != 0.0, "ke_dropped": True, "use_prev_ignored": not p["use_prev"],
            "suffix_included": q > 0 and statistics_matter}[defect]


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_modelled_defect_leaves_the_bounds(defect):
    hit = 0
    for name, b in CASES:
        if not _applies(defect, name, b):
            continue
        w, extra = R.window(name, b)
        p = R.case_par(name, b)
        f, m_new, e = R.emulate(*w, p, defect, extra=extra)
        assert R.ratio(*w, p, f, m_new, e) > 1.0, (defect, name, b)
        hit += 1
    assert hit >= 2, defect


# ---------------------------------------------------------------- the keywords
def test_projection_vectors():
    assert projection_vectors(None, None, None, 3) is None
    eta, r, beta = projection_vectors(0.5, None, None, 3)
    assert eta.tolist() == [0.5] * 3 and r.tolist() == [0.0] * 3 and beta.tolist() == [0.0] * 3 and eta.dtype == torch.float32
    eta, r, beta = projection_vectors([0.0, 1.0], 2.5, torch.tensor([-0.5, 0.25]), 2)
    assert eta.tolist() == [0.0, 1.0] and r.tolist() == [2.5, 2.5] and beta.tolist() == [-0.5, 0.25]
    for bad in (-0.1, 1.5, float("nan"), True, "a", [0.5, 2.0, 0.1], [0.5, None, 0.1]):
        with pytest.raises(ValueError, match="guidance_projection"):
            projection_vectors(bad, None, None, 3)
    for bad in (0.0, -1.0, float("inf"), True, [1.0, 0.0, 2.0]):
        with pytest.raises(ValueError, match="guidance_norm_threshold"):
            projection_vectors(0.5, bad, None, 3)
    for bad in (1.0, -1.0, 1.5, float("nan"), True, [0.0, -1.0, 0.0]):
        with pytest.raises(ValueError, match="guidance_momentum"):
            projection_vectors(0.5, None, bad, 3)
    for bad in ([0.5, 0.5], [0.1] * 4):
        with pytest.raises(ValueError, match="3 values expected"):
            projection_vectors(bad, None, None, 3)
    with pytest.raises(ValueError, match="guidance_norm_threshold needs guidance_projection"):
        projection_vectors(None, 2.0, None, 3)
    with pytest.raises(ValueError, match="guidance_momentum needs guidance_projection"):
        projection_vectors(None, None, -0.5, 3)


def test_project_table():
    ac = torch.linspace(0.999, 0.01, 50, dtype=torch.float64)
    rows = multistep_schedule(ac, 5)
    t = project_table(projection_vectors([0.0, 1.0], 2.5, -0.5, 2), guidance_vector([5.0, 3.0], 2), rows, [False, True, False, True, True])
    assert t.shape == (5, 2, 8) and t.dtype == torch.float32
    for i, row in enumerate(rows):
        assert t[i, :, 0].tolist() == [np.float32(row[2])] * 2 and t[i, :, 1].tolist() == [np.float32(row[3])] * 2
        assert t[i, :, 2].tolist() == [5.0, 3.0] and t[i, :, 3].tolist() == [0.0, 1.0]
        assert t[i, :, 4].tolist() == [2.5, 2.5] and t[i, :, 5].tolist() == [-0.5, -0.5]
    # use_prev: from the second guided step on, across the unguided step in between
    assert t.view(torch.int32)[:, :, 6].tolist() == [[0, 0], [0, 0], [0, 0], [1, 1], [1, 1]]
    assert t.view(torch.int32)[:, :, 7].abs().sum() == 0


def test_closed_call_refusals_before_any_launch():
    sg = _bare_generator(DiTTOConfig(256, 2, 4, 256, 256, 50))
    audio, text = torch.zeros(15, 256), torch.zeros(9, 256)
    packed = (text, [0, 3, 6, 9], audio, [0, 5, 6, 15])
    ok = dict(guidance=2.0, null_text_emb=text)
    for solver in ("ddim", "dpmpp2m"):
        for kw, word in ((dict(guidance_projection=1.5), "guidance_projection"), (dict(guidance_projection=[0.5, 0.5]), "3 values"),
                         (dict(guidance_projection=0.5, guidance_norm_threshold=0.0), "guidance_norm_threshold"),
                         (dict(guidance_projection=0.5, guidance_momentum=1.0), "guidance_momentum"),
                         (dict(guidance_norm_threshold=2.0), "needs guidance_projection"),
                         (dict(guidance_momentum=-0.5), "needs guidance_projection")):
            with pytest.raises(ValueError, match=word):
                sg.sample_guided_packed(*packed, solver=solver, **kw, **ok)
        with pytest.raises(ValueError, match="guidance_projection needs guidance"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_projection=0.5)
        with pytest.raises(ValueError, match="guidance_projection needs guidance"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_projection=0.5, guidance=2.0)
        with pytest.raises(NotImplementedError, match="guidance_rescale"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_projection=0.5, guidance_rescale=0.7, **ok)
        with pytest.raises(NotImplementedError, match="guidance_refresh"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_projection=0.5, guidance_refresh=2, **ok)
    # the padded layouts point to the packed call, as they do for the rescale
    padded = (torch.zeros(1, 3, 256), torch.zeros(1, 5, 256))
    for entry in (sg.sample_guided, sg.sample_latents_strided):
        for kw in (dict(guidance_projection=0.5), dict(guidance_norm_threshold=2.0), dict(guidance_momentum=-0.5)):
            with pytest.raises(NotImplementedError, match="sample_guided_packed"):
                entry(*padded, **kw)
    from ditto_tts_amd.dist import sample_sharded
    with pytest.raises(NotImplementedError, match="sample_guided_packed"):
        sample_sharded(None, None, None, None, None, "cpu", guidance_projection=0.5)
    # the existing refusals stay in front: head_dim != 64 and fp8 linears
    for cfg, word in ((DiTTOConfig(256, 2, 2, 256, 256, 50), "head_dim 64"), (DiTTOConfig(256, 2, 4, 256, 256, 50, fp8_linear=True), "fp8")):
        with pytest.raises(NotImplementedError, match=word):
            _bare_generator(cfg).sample_guided_packed(*packed, guidance_projection=0.5, **ok)
