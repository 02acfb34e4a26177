"""The fp64 reference of projected guidance (Adaptive Projected Guidance: Sadat, Hilliges & Weber 2024, "Eliminating Oversaturation and
Artifacts of High Guidance Scales in Diffusion Models", Algorithm 1) as include/ditto_project.h defines it for packed guided sampling,
the paper's algorithm written out directly, the exact fp32 chains of the kernels, and the DERIVED bounds the GPU tests hold them to.

Contract, per utterance, over its generated window of n elements (x, c, u, m fp32; par = kx, ke, w, eta, r, beta, use_prev):
    dd = ke (c - u);  m' = use_prev ? beta m + dd : dd;  D = kx x + ke c
    S_mm = sum m'^2, S_mD = sum m' D, S_DD = sum D^2
    rms = sqrt(S_mm / n);  rho = r / rms if r > 0 and rms is finite and > r, else 1;  p = S_mD / S_DD if S_DD finite and > 0, else 0
    kappa = (w - 1) rho (1 - eta) p;  fx = -kappa kx / ke,  fc = 1 - kappa,  fd = (w - 1) rho / ke;  ke == 0: (0, 1, 0)
    e = fx x + fc c + fd m'
The library evaluates dd = ke * (c - u), m' = fmaf(beta, m, dd), D = fmaf(kx, x, ke * c) and e = fmaf(fx, x, fmaf(fc, c, fd * m')) in
fp32, the three sums in fp64 from those fp32 values, the finish in fp64, and casts (fx, fc, fd) to fp32.

Bounds.  eps = 2^-24 (the unit roundoff of fp32), first order in eps unless said; |.| elementwise, ||.|| the 2-norm over the window.
  * dm_i = |m'^_i - m'_i| <= 2 eps |dd_i| (the rounding of c - u scaled by ke, and the rounding of the product) + eps |m'_i| with
    use_prev (the one rounding of the fma);
  * dD_i = |D^_i - D_i| <= eps |ke c_i| + eps |D_i| (the product, then the fma);
  * a norm is 1-Lipschitz: | ||m'^|| - ||m'|| | <= ||dm||, so rms^ has relative error a_m = ||dm|| / ||m'||, and likewise a_D = ||dD|| /
    ||D|| for ||D^||, i.e. 2 a_D + a_D^2 for S_DD;
  * |S_mD^ - S_mD| <= ||dm|| ||D|| + ||m'|| ||dD|| + ||dm|| ||dD||  (Cauchy-Schwarz on each cross term);
  * the fp64 accumulation: as in tests/rescale_ref.py every sum passes through fewer than 3000 fp64 roundings in a row — relative
    error below ACC64 = 1e-12 of sum |terms|: of the sum itself for S_mm and S_DD, of ||m'|| ||D|| for S_mD; the few fp64 operations
    of the finish are covered by the same ACC64 on each factor;
  * rho: 0 where the threshold is off or clearly inactive; else d_rho = rho rel / (1 - rel) with rel = a_m + ACC64 (this also covers
    the branch flipping when rms is within rel of r: min(1, r / rms) is continuous);
  * p: d_p = (E_mD / S_DD + |p| rel_DD) / (1 - rel_DD), E_mD the S_mD bound plus ACC64 ||m'|| ||D||, rel_DD = 2 a_D + a_D^2 + ACC64;
  * kappa: d_k = |w - 1| (1 - eta) (d_rho |p| + rho d_p + d_rho d_p) + ACC64 |kappa|;
  * the casts: d_fx = |kx / ke| d_k + (eps + ACC64) |fx|;  d_fc = d_k + eps |fc|;  d_fd = |w - 1| d_rho / |ke| + (eps + ACC64) |fd|;
  * e: de_i = d_fx |x_i| + d_fc |c_i| + d_fd (|m'_i| + dm_i) + |fd| dm_i                    (the coefficients and the stored m')
             + eps |fd m'_i| + eps |fc c_i + fd m'_i| + eps |e_i|                            (the product and the two fmas).
  * orthogonality (eta = 0, beta = 0, r off): with D = kx x + ke e and D_c = kx x + ke c, <D - D_c, D_c> = 0 exactly; from the
    library's e^, <D^ - D_c, D_c> = ke <e^ - e, D_c>, so |.| <= |ke| sum de_i |D_c,i|.
Nothing here comes from what the kernels return.
"""
import functools

import numpy as np

EPS32 = 2.0 ** -24
ACC64 = 1e-12
CHUNK_QUADS = 4096          # DITTO_RESCALE_CHUNK_QUADS: quads per partial of the kernels

PAR_FIELDS = ("kx", "ke", "w", "eta", "r", "beta", "use_prev")
KX_EPS, KE_EPS = 1.9160, -1.6344          # multistep_schedule's (1 / alpha, -sigma / alpha) at a mid timestep
KX_V, KE_V = 0.6, -0.8                    # multistep_schedule_v's (alpha, -sigma)


def par(kx, ke, w, eta, r=0.0, beta=0.0, use_prev=0):
    """one utterance's parameters, each rounded to the fp32 value the device struct holds"""
    f = lambda v: float(np.float32(v))
    return dict(kx=f(kx), ke=f(ke), w=f(w), eta=f(eta), r=f(r), beta=f(beta), use_prev=int(use_prev))


def _f64(*arrs):
    return [np.asarray(a, np.float64).ravel() for a in arrs]


def _finish(S_mm, S_mD, S_DD, n, p_):
    """the finish in fp64 -> (fx, fc, fd, rho, p, kappa)"""
    if p_["ke"] == 0.0:
        return 0.0, 1.0, 0.0, 1.0, 0.0, 0.0
    rms = np.sqrt(S_mm / n)
    rho = p_["r"] / rms if (p_["r"] > 0.0 and np.isfinite(rms) and rms > p_["r"]) else 1.0
    p = S_mD / S_DD if (np.isfinite(S_DD) and S_DD > 0.0) else 0.0
    eta = min(max(p_["eta"], 0.0), 1.0) if p_["eta"] == p_["eta"] else 0.0
    wr = (p_["w"] - 1.0) * rho
    kappa = (wr * (1.0 - eta)) * p
    return (-kappa * p_["kx"]) / p_["ke"], 1.0 - kappa, wr / p_["ke"], rho, p, kappa


def reference(x, c, u, m, p_):
    """The contract in fp64 from fp32 inputs -> dict(fx, fc, fd, rho, p, kappa, m_new, D, dd, e)"""
    x, c, u, m = _f64(x, c, u, m)
    dd = p_["ke"] * (c - u)
    m_new = p_["beta"] * m + dd if p_["use_prev"] else dd
    D = p_["kx"] * x + p_["ke"] * c
    fx, fc, fd, rho, p, kappa = _finish(float(m_new @ m_new), float(m_new @ D), float(D @ D), float(x.size), p_)
    return dict(fx=fx, fc=fc, fd=fd, rho=rho, p=p, kappa=kappa, m_new=m_new, D=D, dd=dd, e=fx * x + fc * c + fd * m_new)


def apg_direct(x, c, u, m, p_):
    """The paper's Algorithm 1 written out directly in fp64 — both x0 predictions, their difference, the momentum, the threshold (on
    the RMS: the one documented deviation), decompose, scale, recombine — and back to the network's output space -> (e, m_new)"""
    x, c, u, m = _f64(x, c, u, m)
    D_c, D_u = p_["kx"] * x + p_["ke"] * c, p_["kx"] * x + p_["ke"] * u
    diff = D_c - D_u
    if p_["use_prev"]:
        diff = diff + p_["beta"] * m                       # the running average: kept BEFORE thresholding
    m_new = diff.copy()
    if p_["r"] > 0.0:
        rms = np.sqrt(np.mean(diff * diff))
        diff = diff * min(1.0, p_["r"] / rms)
    par_ = (diff @ D_c) / (D_c @ D_c) * D_c
    orth = diff - par_
    D = D_c + (p_["w"] - 1.0) * (orth + p_["eta"] * par_)
    return (D - p_["kx"] * x) / p_["ke"], m_new


def bounds(x, c, u, m, p_):
    """-> dict(fx, fc, fd: bounds on the fp32 coefficients against reference(); m: elementwise bound on the stored m'; e: elementwise
    bound on the library's e given ITS coefficients lie inside theirs) — see the module docstring"""
    ref = reference(x, c, u, m, p_)
    x, c, u, m = _f64(x, c, u, m)
    mn, D = ref["m_new"], ref["D"]
    dm = 2.0 * EPS32 * np.abs(ref["dd"]) + (EPS32 * np.abs(mn) if p_["use_prev"] else 0.0)
    dD = EPS32 * np.abs(p_["ke"] * c) + EPS32 * np.abs(D)
    nm, nD, ndm, ndD = (float(np.sqrt(v @ v)) for v in (mn, D, dm, dD))
    assert nm > 0.0 and nD > 0.0, "the bound needs a direction and a prediction away from 0"
    a_m, a_D = ndm / nm, ndD / nD
    rel_m, rel_DD = a_m + ACC64, 2.0 * a_D + a_D * a_D + ACC64
    rms = nm / np.sqrt(x.size)
    d_rho = ref["rho"] * rel_m / (1.0 - rel_m) if (p_["r"] > 0.0 and rms > p_["r"] * (1.0 - 2.0 * rel_m)) else 0.0
    E_mD = ndm * nD + nm * ndD + ndm * ndD + ACC64 * nm * nD
    d_p = (E_mD / (nD * nD) + abs(ref["p"]) * rel_DD) / (1.0 - rel_DD)
    eta, wm1 = min(max(p_["eta"], 0.0), 1.0), abs(p_["w"] - 1.0)
    d_k = wm1 * (1.0 - eta) * (d_rho * abs(ref["p"]) + ref["rho"] * d_p + d_rho * d_p) + ACC64 * abs(ref["kappa"])
    d_fx = abs(p_["kx"] / p_["ke"]) * d_k + (EPS32 + ACC64) * abs(ref["fx"])
    d_fc = d_k + EPS32 * abs(ref["fc"])
    d_fd = wm1 * d_rho / abs(p_["ke"]) + (EPS32 + ACC64) * abs(ref["fd"])
    fd, fc = ref["fd"], ref["fc"]
    de = (d_fx * np.abs(x) + d_fc * np.abs(c) + d_fd * (np.abs(mn) + dm) + abs(fd) * dm
          + EPS32 * (np.abs(fd * mn) + np.abs(fc * c + fd * mn) + np.abs(ref["e"])))
    return dict(fx=d_fx, fc=d_fc, fd=d_fd, m=dm, e=de, ref=ref)


def ortho_bound(x, c, u, m, p_):
    """bound on |<D^ - D_c, D_c>| for eta = 0, beta = 0, r off, D^ = kx x + ke e^ from the library's e^"""
    b = bounds(x, c, u, m, p_)
    return abs(p_["ke"]) * float(b["e"] @ np.abs(b["ref"]["D"]))


# ---------------------------------------------------------------- the kernels' fp32 chains, exactly
def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 arrays, exactly: the product of two fp32 numbers is exact in fp64; the fp64 sum is rounded TO ODD
    (TwoSum gives its error), after which the rounding to fp32 is the correct single rounding (53 >= 24 + 2 bits)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) != 0
        fix = (err != 0.0) & ~odd & np.isfinite(s) & np.isfinite(err)
        s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def direction32(x, c, u, m, p_):
    """launch 1's fp32 values -> (m' fp32, D fp32): the bits the kernel stores and sums"""
    x, c, u, m = (np.asarray(v, np.float32).ravel() for v in (x, c, u, m))
    kx, ke, beta = np.float32(p_["kx"]), np.float32(p_["ke"]), np.float32(p_["beta"])
    with np.errstate(invalid="ignore"):
        dd = ke * (c - u)
        m_new = fma32(beta, m, dd) if p_["use_prev"] else dd
        return m_new, fma32(kx, x, ke * c)


def e32(x, c, m_new, f):
    """launch 2's guided prediction from fp32 coefficients f = (fx, fc, fd): fmaf(fx, x, fmaf(fc, c, fd * m'))"""
    x, c, m_new = (np.asarray(v, np.float32).ravel() for v in (x, c, m_new))
    fx, fc, fd = (np.float32(v) for v in f[:3])
    with np.errstate(invalid="ignore"):
        return fma32(fx, x, fma32(fc, c, fd * m_new))


DEFECTS = ("project_on_u", "norm_not_rms", "threshold_into_m", "beta_sign", "ke_dropped", "use_prev_ignored", "suffix_included")


def emulate(x, c, u, m, p_, defect=None, extra=None):
    """The kernels' arithmetic on the host — direction32, the three sums in fp64 in numpy's order, the finish, the casts, e32 — with
    one modelled defect, or none -> (f fp32 [3], m' fp32, e fp32).  `extra`: (x, c, u, m) of the suffix rows, for "suffix_included"."""
    assert defect is None or defect in DEFECTS
    q = dict(p_)
    if defect == "beta_sign":
        q["beta"] = -q["beta"]
    if defect == "use_prev_ignored":
        q["use_prev"] = 1
    if defect == "ke_dropped":
        x32, c32, u32, m32 = (np.asarray(v, np.float32).ravel() for v in (x, c, u, m))
        dd = c32 - u32
        m_new = fma32(np.float32(q["beta"]), m32, dd) if q["use_prev"] else dd
        D = fma32(np.float32(q["kx"]), x32, np.float32(q["ke"]) * c32)
    else:
        m_new, D = direction32(x, c, u, m, q)
    sm, sD = m_new.astype(np.float64), D.astype(np.float64)
    if defect == "project_on_u":
        sD = direction32(x, u, u, m, q)[1].astype(np.float64)
    if defect == "suffix_included":
        em, eD = direction32(*extra, q)
        sm, sD = np.concatenate([sm, em.astype(np.float64)]), np.concatenate([sD, eD.astype(np.float64)])
    n = float(sm.size)
    S_mm, S_mD, S_DD = float(np.sum(sm * sm)), float(np.sum(sm * sD)), float(np.sum(sD * sD))
    if defect == "norm_not_rms":
        n = 1.0
    fx, fc, fd, rho, _, _ = _finish(S_mm, S_mD, S_DD, n, q)
    if defect == "threshold_into_m":
        m_new = (np.float32(rho) * m_new).astype(np.float32)
    f = np.array([fx, fc, fd], np.float32)
    return f, m_new, e32(x, c, m_new, f)


def ratio(x, c, u, m, p_, f, m_new, e):
    """how far (f, m', e) stand from the fp64 reference in units of their bounds: the largest of the three coefficients', the stored
    direction's and e's elementwise ratios; NaN anywhere counts as infinitely far.  <= 1: inside every bound"""
    b = bounds(x, c, u, m, p_)
    ref = b["ref"]
    tiny = 1e-300
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = [abs(float(f[i]) - ref[k]) / max(b[k], tiny) for i, k in enumerate(("fx", "fc", "fd"))]
        rs.append(float(np.max(np.abs(np.asarray(m_new, np.float64) - ref["m_new"]) / np.maximum(b["m"], tiny))))
        rs.append(float(np.max(np.abs(np.asarray(e, np.float64) - ref["e"]) / np.maximum(b["e"], tiny))))
    return float("inf") if any(r != r for r in rs) else max(rs)


# ---------------------------------------------------------------- the GPU kernel test's own inputs
# four parameter sets: both coefficient pairs, r off / on (inactive: 50 is far above any RMS here, and far below the norm of all but
# the shortest windows; active: 0.25 is half the RMS of dd under KE_V), beta 0 and -0.5, use_prev 0 (the test fills m with NaN there)
PARS = (par(KX_EPS, KE_EPS, 5.0, 0.3, r=50.0, beta=-0.5, use_prev=1),
        par(KX_V, KE_V, 4.0, 0.0, r=0.25, beta=0.0, use_prev=0),
        par(KX_EPS, KE_EPS, 5.0, 1.0, r=0.0, beta=0.0, use_prev=0),       # plain classifier-free guidance
        par(KX_V, KE_V, 3.0, 0.0, r=0.0, beta=0.0, use_prev=1))           # the orthogonality case
# name -> (d, [(generated rows, prompt rows, suffix rows)] x 4, the utterances' parameter sets): a chunk is 4096 quads = 16384 elements
# = 256 rows of 64 = 64 rows of 256 = 21 1/3 rows of 768.  Every shape meets every set; set 0 (r = 50) always sits on a window whose
# norm is far above 50
SHAPES = {"d64": (64, [(1, 0, 0), (256, 0, 0), (257, 0, 0), (3, 0, 0)], (1, 0, 3, 2)),
          "d768": (768, [(22, 0, 0), (70, 0, 0), (1, 0, 0), (43, 0, 0)], (2, 3, 1, 0)),
          "d256": (256, [(5, 3, 2), (64, 0, 4), (65, 7, 0), (17, 2, 9)], (3, 1, 0, 2))}


def case_par(name, b):
    """the parameter set utterance b of shape `name` runs with"""
    return PARS[SHAPES[name][2][b]]


@functools.lru_cache(maxsize=None)
def rows(name, b):
    """utterance b of shape `name`: (x, c, u, m) fp32 numpy [n_b, d] over ALL its rows (prompt, window, suffix), a function of the
    utterance alone; c and u correlated, as the two halves of a guided forward are; m is NaN where the utterance's use_prev is 0"""
    from ditto_tts_amd.synth import hash_normal
    d, utts, _ = SHAPES[name]
    g, p, q = utts[b]
    n, key = g + p + q, 1000 * (sorted(SHAPES).index(name) + 1) + b
    x, c, nz, m = (hash_normal((n, d), tag, key) for tag in ("pj_x", "pj_c", "pj_u", "pj_m"))
    m = (0.7 * m).numpy()
    if not case_par(name, b)["use_prev"]:
        m = np.full_like(m, np.nan)
    return x.numpy(), c.numpy(), (0.8 * c + 0.6 * nz).numpy(), m


def window(name, b):
    """(x, c, u, m) over utterance b's generated window alone, and over its suffix rows"""
    g, p, q = SHAPES[name][1][b]
    full = rows(name, b)
    return tuple(v[p:p + g] for v in full), tuple(v[p + g:] for v in full)
