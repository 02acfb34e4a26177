"""The fp64 reference of guidance rescale (Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section
3.4) as include/ditto_hip.h defines it for packed guided sampling, and the DERIVED bound the GPU tests hold the kernels to.

Definition, per guided utterance, over its generated rows and all d columns (c, u: the conditional / unconditional eps, fp32):
    e_i = u_i + w (c_i - u_i)                                   (the library evaluates fmaf(w, c_i - u_i, u_i) in fp32)
    sigma_c, sigma_e = the standard deviations of c and e       (population form; the ratio below does not depend on the n / (n - 1)
                                                                 convention — both variances carry the same factor — see test_rescale_ref)
    r = sigma_c / sigma_e,  s = 1 + phi (r - 1),  s32 = (float)s,  coef_out = coef_in * s32 (one fp32 multiply)
    s32 = 1 exactly (coef_out a bit copy) where phi == 0, the utterance is unguided, sigma_e^2 <= 0 or r is not finite.

Bound.  With eps = 2^-24 (the unit roundoff of fp32):
  * the fp32 evaluation of e_i is off by at most delta_i = eps (|w| |c_i - u_i| + |e_i|): one rounding of c_i - u_i, scaled by w, and
    the one rounding of the fused multiply-add (second-order terms eps^2 dropped);
  * the standard deviation is a seminorm (the 2-norm of the centred vector over sqrt(n)), so |sigma_e^ - sigma_e| <= rms(delta);
  * with rho = rms(delta) / sigma_e:  |r^ - r| <= r rho / (1 - rho);
  * the fp64 accumulation: every sum the kernels form passes through fewer than 3000 fp64 roundings in a row (64 serial adds per lane
    and chunk, a 6-step butterfly, 3 wave adds, then at most ceil(chunks / 64) + 6 in the finish), i.e. relative error below 3000 x
    2^-53 = 3.4e-13 of sum |x| resp. sum x^2; var = E[x^2] - mean^2 then carries a relative error below 1e-12 (1 + mean^2 / var)
    (the cancellation of the one-pass form), and so does r through sqrt(var_c / var_e), once for c and once for e:
        acc = 1e-12 ((1 + mean_c^2 / var_c) + (1 + mean_e^2 / var_e));
  * |s32 - s| <= phi r (rho / (1 - rho) + acc) + eps s                       (the last term: the conversion of s to fp32)
  * |coef_out - coef_in s| <= |coef_in| (that + eps s)                       (the one fp32 multiply).
Nothing here comes from what the kernels return.
"""
import numpy as np

EPS32 = 2.0 ** -24
ACC64 = 1e-12
CHUNK_QUADS = 4096          # DITTO_RESCALE_CHUNK_QUADS: quads per partial of the kernels (used by the emulation's second order only)


def guided_fp64(c, u, w):
    """e = u + w (c - u) in fp64 from fp32 inputs"""
    c, u = np.asarray(c, np.float64).ravel(), np.asarray(u, np.float64).ravel()
    return u + float(w) * (c - u)


def reference(c, u, w, phi, guided=True, ddof=0):
    """-> dict(s=, r=, var_c=, var_e=, mean_c=, mean_e=) in fp64; s == 1.0 exactly in the degenerate cases"""
    c64 = np.asarray(c, np.float64).ravel()
    e = guided_fp64(c, u, w)
    out = dict(s=1.0, r=float("nan"), var_c=float(np.var(c64, ddof=ddof)) if c64.size > ddof else 0.0,
               var_e=float(np.var(e, ddof=ddof)) if e.size > ddof else 0.0, mean_c=float(c64.mean()), mean_e=float(e.mean()))
    phi = min(max(float(phi), 0.0), 1.0)
    if not guided or phi == 0.0 or not out["var_e"] > 0.0:
        return out
    r = float(np.sqrt(out["var_c"] / out["var_e"]))
    if not np.isfinite(r):
        return out
    out["r"], out["s"] = r, 1.0 + phi * (r - 1.0)
    return out


def bound(c, u, w, phi, guided=True):
    """(bound on |s32 - s|, bound on |coef_out - coef_in s| per unit |coef_in|) — see the module docstring"""
    ref = reference(c, u, w, phi, guided)
    if np.isnan(ref["r"]):
        return 0.0, 0.0                                            # the degenerate cases are exact
    c64, u64 = np.asarray(c, np.float64).ravel(), np.asarray(u, np.float64).ravel()
    e = guided_fp64(c, u, w)
    delta = EPS32 * (abs(float(w)) * np.abs(c64 - u64) + np.abs(e))
    rho = float(np.sqrt(np.mean(delta * delta))) / float(np.sqrt(ref["var_e"]))
    assert rho < 0.5, "the bound needs sigma_e well away from 0"
    acc = ACC64 * (2.0 + ref["mean_c"] ** 2 / max(ref["var_c"], 1e-300) + ref["mean_e"] ** 2 / ref["var_e"])
    phi = min(max(float(phi), 0.0), 1.0)
    bs = phi * ref["r"] * (rho / (1.0 - rho) + acc) + EPS32 * ref["s"]
    return bs, bs + EPS32 * ref["s"]


def emulate(c, u, w, phi, order="pairwise"):
    """The kernels' arithmetic on the host, summed in ANOTHER order: e in fp32 as fmaf(w, c - u, u) (the product w (c - u) is exact
    in fp64 — 24 x 24 bits —, so adding u there and rounding to fp32 differs from a true fma only in a last-bit tie of the double
    rounding, far inside delta), the four sums in fp64, var = E[x^2] - mean^2, r, s, (float)s.  order: "pairwise" (numpy's), "reverse"
    (serial from the last element) or "chunks" (serial inside chunks of CHUNK_QUADS quads, then over the chunks)."""
    c32, u32 = np.asarray(c, np.float32).ravel(), np.asarray(u, np.float32).ravel()
    t = (c32 - u32).astype(np.float32)
    e32 = (np.float64(np.float32(w)) * t.astype(np.float64) + u32.astype(np.float64)).astype(np.float32)
    cd, ed = c32.astype(np.float64), e32.astype(np.float64)

    def total(x):
        if order == "pairwise":
            return float(np.sum(x))
        if order == "reverse":
            return float(np.cumsum(x[::-1])[-1])
        parts = [float(np.cumsum(x[k:k + 4 * CHUNK_QUADS])[-1]) for k in range(0, x.size, 4 * CHUNK_QUADS)]
        return float(np.cumsum(np.asarray(parts))[-1])

    n = float(cd.size)
    mc, me = total(cd) / n, total(ed) / n
    vc, ve = max(total(cd * cd) / n - mc * mc, 0.0), total(ed * ed) / n - me * me
    phi = min(max(float(np.float32(phi)), 0.0), 1.0)
    if phi == 0.0 or not ve > 0.0:
        return np.float32(1.0)
    r = np.sqrt(vc / ve)
    if not np.isfinite(r):
        return np.float32(1.0)
    return np.float32(1.0 + phi * (r - 1.0))
