"""The fused attention backward's fp64 reference, an elementwise error bound derived from the two kernels' arithmetic, a CPU model of
that arithmetic with the bugs the bound must catch, and the test data (plain helpers, shared by test_attention_bwd_bound.py and
test_gpu_attention_bwd_elementwise.py; U, G and worst_ratio are attn_ref.py's).

The backward (csrc/attn64bwd.h) is a function of (q, k, v, dO, O, L, scale, p, seed, layer, rope tables): L is the forward's
log2-domain log-sum-exp per (head, query), O its output.  Per (utterance, head), with c = fp32(scale) * fp32(log2 e) and
km = keep mask / (1 - p) (1 without dropout):

    dq kernel (MODE 0)     q' = bf16(fp32(q) c),  P = exp2(q'.k - L_i)       (the score chain starts from -L: fp32 MFMA sums)
    dk,dv kernel (MODE 1)                         P = exp2(c (q.k) - L_i)    (raw q tile, the product scaled per element)
    both                   dP = dO V^T,  delta_i = sum_c dO_ic O_ic,  x = dP km - delta,  dS' = P x
    dQ = scale dS' K       dK = scale dS'^T q (raw q)       dV = (P km)^T dO
    rope tables given      (dQ, dK) rows get the inverse half-split rotation at the row's position inside its utterance

The two P differ by 2^d_ij, d_ij = (c q_i - q'_i).k_j: reference() follows each kernel's own formula (qprime_dkdv=True gives the
other definition for dk / dv, to measure how far apart they are).

THE BOUND, term by term (u = U = 2^-8 bf16 roundoff, G = 2^-24; every fp32 sum of the matrix pipe is charged 2 G per term: its
internal rounding is not documented as round-to-nearest):
  score   64 products and the -L start (MODE 0) / 64 products, the factor c and the subtraction of L (MODE 1), in fp32:
          |ds_ij| <= 2 G (dh + 2) a_ij,  a_ij = sum_c |q_ic k_jc| (log2 units) + |L_i|.  L itself is an fp32 operand, taken as
          given; what it costs is this subtraction's rounding at the magnitude of L.
  exp     v_exp_f32: EXP = 2^-22 relative (one ulp of the documented accuracy, doubled).
          => P is off by rho_ij = ln2 |ds_ij| + EXP, relatively.
  dP      64 fp32 products: |d dP_ij| <= 2 G dh sum_c |dO_ic v_jc|.
  delta   64 fp32 products (plain fp32 adds and one exchange): |d delta_i| <= G dh sum_c |dO_ic O_ic|.
  x       dP km - delta in fp32 (two roundings, or one fused): <= 2 G (|dP km| + |delta|).  This is where the cancellation lives:
          ex_ij = km |d dP| + |d delta| + 2 G (|dP km| + |delta|) is ABSOLUTE, in terms of |dP km| + |delta|, never of |x|.
  dS'     P x rounded to fp32 then bf16: E_ij = P (1 + rho + 2 u) ((rho + u + 4 G) |x| + ex)  bounds |dS'_hat - dS'|.
  P km    rounded to fp32 then bf16 (dV's operand): Ev_ij = P km (1 + rho) (rho + u + 2 G).
  sums    the accumulating MFMAs add n terms in fp32, n = the tile-padded Skv (dq) or Sq (dk, dv): 2 G (n + 8) sum |terms|.
  scale   one fp32 product on the accumulators (dq, dk); G relative, charged as 2 G |result|.
    |dQ_hat - dQ| <= scale (E |K| + 2 G (n + 8) (|dS'| + E) |K|) + 2 G |dQ|      (likewise dK with |q|, dV with Ev and |dO|)
  rope    lo' = lo cos + hi sin, hi' = hi cos - lo sin in fp32 on the accumulators: a pair's bounds map through |cos| and |sin|, plus
          4 G (|lo cos| + |hi sin|) for the two products and the sum.
No element is excluded.  A result stored as bf16 adds half an ulp of itself (granted by worst_ratio(stored_bf16=True)).  A single
rounding attains u, so an output that is ONE product (dk, dv with one query; dq with one key) can come arbitrarily close to ratio 1."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from attn_ref import G, LOG2E, U, worst_ratio   # noqa: F401  (worst_ratio re-exported for the tests)
from gpu_util import asym
from oracle import ditto_oracle as O

DH = 64
EXP = 2.0 ** -22
SEED, LAYER = 0x1234567890ABCDEF, 3

# (B, H, Sq, Skv): the smallest shapes at which each mechanism of the kernels exists
DENSE = [(1, 1, 64, 64),      # one whole tile, no-mask instantiation
         (2, 3, 100, 72),     # ragged both sides, batch rows not tile-aligned, bh indexing of lse / stats
         (1, 2, 130, 650),    # 11 key tiles: the ring wraps twice, ragged tail, a third query block of two valid rows
         (1, 1, 710, 64),     # 12 query tiles for the dk,dv ring, ragged query tail
         (1, 2, 256, 192),    # whole tiles (with dropout: the no-mask DROP instantiation)
         (1, 2, 3, 1),        # single key
         (1, 2, 1, 130)]      # single query
EXCHANGE = (1, 2, 130, 130)   # L of the two heads exchanged
# (QL, KL, H) of test_packed_attention_forward_and_backward_vs_autograd, with one utterance of length 1 put second
PACKED_CROSS = [([40, 1, 100, 128, 70], [1, 1, 72, 64, 130], 2), ([64, 1, 130], [650, 1, 33], 1), ([710, 1, 20], [64, 1, 90], 1)]
PACKED_SELF = [([40, 1, 192, 100, 257], 2), ([704, 1, 33], 1)]


def dense_segs(B, Sq, Skv):
    return [(b * Sq, Sq, b * Skv, Skv) for b in range(B)]


def packed_segs(QL, KL):
    segs, q0, k0 = [], 0, 0
    for nq, nk in zip(QL, KL):
        segs.append((q0, nq, k0, nk))
        q0, k0 = q0 + nq, k0 + nk
    return segs


def _f32(x):
    return float(np.float32(x))


def _c32(scale):
    return float(np.float32(scale) * np.float32(LOG2E))


def keep_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def q_prime(q, scale):
    """bf16(fp32(q) * c32): the dq kernel's (and the training forward's) query operand"""
    return (q.float() * torch.tensor(_c32(scale), dtype=torch.float32)).to(torch.bfloat16)


def _cols(h):
    return slice(h * DH, (h + 1) * DH)


def _blocks(case):
    for b, (q0, nq, k0, nk) in enumerate(case.segs):
        for h in range(case.H):
            yield b, h, slice(q0, q0 + nq), slice(k0, k0 + nk), _cols(h)


def make_case(segs, H, seed, p=0.0, rope=False, sharp=2.5, late=True):
    """UNSCALED bf16 q, bf16 k, v, dO [rows, H * 64]; natural-log logits of std `sharp`, and (late) two rows of every (utterance, head)
    long enough with one key +40 / +30 log2 units above the rest, as attn_ref.make_case.  p > 0: keep, the hash keep-mask at
    utterance-local indices on a square large enough for a padded tile and for (query, key) swapped.  rope: cos / sin [rows, 32] at
    EVERY global row (the kernel is handed the first max_q rows).  L, O: the "supplied" statistics — the fp64 log2-domain
    log-sum-exp of q'.k rounded to fp32, and the fp64 output (P km) V rounded to bf16 — so the backward can be driven without the forward."""
    Rq, Rk = segs[-1][0] + segs[-1][1], segs[-1][2] + segs[-1][3]
    scale = 1.0 / math.sqrt(DH)
    q = asym((Rq, H * DH), seed) * sharp
    k = asym((Rk, H * DH), seed + 1)
    v = asym((Rk, H * DH), seed + 2)
    dO = asym((Rq, H * DH), seed + 3)
    for q0, nq, k0, nk in segs:
        if late and nk > 70 and nq > 9:
            for h in range(H):
                for row, key, lg2 in ((5, nk - 3, 40.0), (9, 70, 30.0)):
                    qr = q[q0 + row, _cols(h)]
                    k[k0 + key, _cols(h)] = qr * (lg2 / (LOG2E * scale * float(qr @ qr)))
    c = SimpleNamespace(segs=segs, H=H, Rq=Rq, Rk=Rk, scale=scale, p=p, keep=None, cos=None, sin=None,
                        maxq=max(s[1] for s in segs), maxk=max(s[3] for s in segs))
    c.q, c.k, c.v, c.dO = (t.to(torch.bfloat16) for t in (q, k, v, dO))
    if p > 0:
        M = 64 * ((max(c.maxq, c.maxk) + 63) // 64)
        c.keep = O.hash_dropout_mask(SEED, LAYER, len(segs), H, M, M, p)
    if rope:
        pos = O.rotary_table(O.rotary_inv_freq(DH), Rq)[:, :DH // 2]
        c.cos, c.sin = torch.cos(pos).contiguous(), torch.sin(pos).contiguous()
    qp = q_prime(c.q, scale)
    c.L = torch.empty(H, Rq, dtype=torch.float32)
    c.O = torch.empty(Rq, H * DH, dtype=torch.bfloat16)
    for b, h, qs, ks, cl in _blocks(c):
        S = qp[qs, cl].double() @ c.k[ks, cl].double().T
        m = S.amax(1, keepdim=True)
        L = m[:, 0] + torch.log2(torch.exp2(S - m).sum(1))
        W = torch.exp2(S - L[:, None]) * _km(c, b, h, S.shape)
        c.L[h, qs] = L.float()
        c.O[qs, cl] = (W @ c.v[ks, cl].double()).to(torch.bfloat16)
    return c


def _km(case, b, h, shape, swapped=False):
    """keep mask / (1 - p) of block (b, h) as fp64 [nq, nk] (ones without dropout); swapped: the mask of (key, query)"""
    if case.keep is None:
        return torch.ones(shape, dtype=torch.float64)
    nq, nk = shape
    m = case.keep[b, h, :nk, :nq].T if swapped else case.keep[b, h, :nq, :nk]
    return m.double() * keep_scale(case.p)


def _unrope(lo, hi, c, s):
    return lo * c + hi * s, hi * c - lo * s


def _rope_rows(case, b, qs, nrows, glob=False):
    """cos, sin of the nrows rows of utterance b: position inside the utterance (glob: the global row, the bug)"""
    r0 = qs.start if glob else 0
    return case.cos[r0:r0 + nrows], case.sin[r0:r0 + nrows]


def reference(case, L, O_, qprime_dkdv=False):
    """fp64 on the exact operands, for the given L [H, Rq] fp32 and O [Rq, H * 64] bf16 whatever produced them: dq, dk, dv and the
    elementwise bounds e_dq, e_dk, e_dv on |got - want| before the bf16 store (module docstring).  The bound's terms are per
    (query, key) — rho_ij, ex_ij weight every product of the sums — so its absolute-value sums (E |K|, |dS'| |K|, ...) are formed here, in
    the same pass over the [nq, nk] matrices, and bound() only hands them out.  qprime_dkdv: dk, dv from the dq kernel's
    probabilities (q' scores throughout), the other definition."""
    H, scale = case.H, _f32(case.scale)
    c32 = _c32(case.scale)
    r = SimpleNamespace(dq=torch.zeros(case.Rq, H * DH, dtype=torch.float64), dk=torch.zeros(case.Rk, H * DH, dtype=torch.float64),
                        dv=torch.zeros(case.Rk, H * DH, dtype=torch.float64))
    r.e_dq, r.e_dk, r.e_dv = torch.zeros_like(r.dq), torch.zeros_like(r.dk), torch.zeros_like(r.dv)
    qp = q_prime(case.q, case.scale)
    for b, h, qs, ks, cl in _blocks(case):
        Q, QP, K, V, DO, OO = (t.double() for t in (case.q[qs, cl], qp[qs, cl], case.k[ks, cl], case.v[ks, cl], case.dO[qs, cl], O_[qs, cl]))
        Lr = L[h, qs].double()[:, None]
        nq, nk = Q.shape[0], K.shape[0]
        km = _km(case, b, h, (nq, nk))
        S0, S1 = QP @ K.T, c32 * (Q @ K.T)
        a0, a1 = QP.abs() @ K.abs().T + Lr.abs(), c32 * (Q.abs() @ K.abs().T) + Lr.abs()
        P0 = torch.exp2(S0 - Lr)
        P1, a1 = (P0, a0) if qprime_dkdv else (torch.exp2(S1 - Lr), a1)
        dP, delta = DO @ V.T, (DO * OO).sum(1, keepdim=True)
        x = dP * km - delta
        ex = km * (2 * G * DH) * (DO.abs() @ V.abs().T) + G * DH * (DO.abs() * OO.abs()).sum(1, keepdim=True) \
            + 2 * G * ((dP * km).abs() + delta.abs())
        nkp, nqp = 64 * ((nk + 63) // 64), 64 * ((nq + 63) // 64)
        out = {}
        for name, P, a in (("dq", P0, a0), ("dkdv", P1, a1)):
            rho = math.log(2.0) * 2 * G * (DH + 2) * a + EXP
            dS = P * x
            E = P * (1 + rho + 2 * U) * ((rho + U + 4 * G) * x.abs() + ex)
            if name == "dq":
                n = 2 * G * (nkp + 8)
                g = scale * (dS @ K)
                e = scale * (E @ K.abs() + n * ((dS.abs() + E) @ K.abs())) + 2 * G * g.abs() + 1e-30
                out["dq"] = (g, e)
            else:
                n = 2 * G * (nqp + 8)
                g = scale * (dS.T @ Q)
                e = scale * (E.T @ Q.abs() + n * ((dS.abs() + E).T @ Q.abs())) + 2 * G * g.abs() + 1e-30
                out["dk"] = (g, e)
                Pk = P * km
                Ev = Pk * (1 + rho) * (rho + U + 2 * G)
                out["dv"] = (Pk.T @ DO, Ev.T @ DO.abs() + n * ((Pk + Ev).T @ DO.abs()) + 1e-30)
        if case.cos is not None:
            for name, rows in (("dq", qs), ("dk", ks)):
                g, e = out[name]
                cs, sn = (t.double() for t in _rope_rows(case, b, rows, g.shape[0]))
                lo, hi = g[:, :32], g[:, 32:]
                glo, ghi = _unrope(lo, hi, cs, sn)
                rnd = 4 * G * ((lo * cs).abs() + (hi * sn).abs()), 4 * G * ((hi * cs).abs() + (lo * sn).abs())
                elo = cs.abs() * e[:, :32] + sn.abs() * e[:, 32:] + rnd[0]
                ehi = cs.abs() * e[:, 32:] + sn.abs() * e[:, :32] + rnd[1]
                out[name] = (torch.cat([glo, ghi], 1), torch.cat([elo, ehi], 1))
        r.dq[qs, cl], r.e_dq[qs, cl] = out["dq"]
        r.dk[ks, cl], r.e_dk[ks, cl] = out["dk"]
        r.dv[ks, cl], r.e_dv[ks, cl] = out["dv"]
    return r


def bound(ref):
    """{name: (want, e)} of a reference(): the elementwise bounds on |got - want| before the bf16 store"""
    return {"dq": (ref.dq, ref.e_dq), "dk": (ref.dk, ref.e_dk), "dv": (ref.dv, ref.e_dv)}


def ratios(got, ref, rows=None):
    """worst ratio of each of got = {dq, dk, dv} (as stored: bf16) against bound(ref); rows: {name: bool row mask} to look at"""
    sel = (lambda n, t: t) if rows is None else (lambda n, t: t[rows[n]])
    return {n: worst_ratio(sel(n, got[n]), sel(n, w), sel(n, e), stored_bf16=True) for n, (w, e) in bound(ref).items()}


def single_product_rows(case):
    """{name: bool row mask} of the outputs that are ONE product: dq rows of an utterance with one key (dS' k), dk / dv rows of an
    utterance with one query (dS' q, (P km) dO).  One bf16 rounding attains u, so there the arithmetic itself can reach ratio 1."""
    one_k, one_q = torch.zeros(case.Rq, dtype=torch.bool), torch.zeros(case.Rk, dtype=torch.bool)
    for q0, nq, k0, nk in case.segs:
        one_k[q0:q0 + nq] = nk == 1
        one_q[k0:k0 + nk] = nq == 1
    return {"dq": one_k, "dk": one_q, "dv": one_q}


STALE_TILE = 5   # a tile whose buffer's previous occupant (tile 1) exists and is a whole tile


def mutations(case):
    """the bugs of emulate() that exist at this case: [(name, outputs on which one of them must show)]"""
    nkt = max((s[3] + 63) // 64 for s in case.segs)
    nqt = max((s[1] + 63) // 64 for s in case.segs)
    m = []
    if nkt > STALE_TILE:
        m.append("stale_key_tile")
    if nqt > STALE_TILE:
        m.append("stale_query_tile")
    # (a single key without dropout has O = v, so dP - delta = 0 on every copy of it: nothing to count)
    if any(s[3] % 64 and (s[3] > 1 or case.p > 0) for s in case.segs):
        m.append("unmasked_tail")
    if nqt > 1:
        m += ["wrong_record", "wrong_delta"]
    if case.H > 1:
        m.append("wrong_L")
    if case.p > 0:
        m.append("no_km_on_dp")
        # (on a block this small the two masks can coincide; the mutation is then the identity)
        if any(not torch.equal(_km(case, b, h, (s[1], s[3])), _km(case, b, h, (s[1], s[3]), swapped=True))
               for b, s in enumerate(case.segs) for h in range(case.H)):
            m.append("swapped_mask")
    if any(s[3] > 1 or case.p > 0 for s in case.segs):   # (a single key without dropout: dS' = 0, dK = 0 whatever its factor)
        m.append("no_scale_on_dk")
    if case.cos is not None:
        m.append("rope_forward")
        if len(case.segs) > 1:
            m.append("rope_global")
    return m


def emulate(case, L, O_, mutate=None):
    """A CPU model of both kernels' arithmetic: bf16 q', fp32 scores, bf16 dS' and P km, fp32 accumulation, fp32 rotation, results in
    fp32 (before the store) — and the bugs the bound must catch:
      stale_key_tile / stale_query_tile   key tile 5 of the dq side (K, V) / query tile 5 of the dk,dv side (q, dO and its {L, delta}
                        record) taken from tile 1, the four-buffer ring's previous occupant
      unmasked_tail     the clamped copies of key Skv - 1 in a ragged last key tile counted by dq
      wrong_record      the neighbouring 64-query tile's {L, delta} record used by dk,dv (wrong_delta: its delta alone)
      wrong_L           L of head (h + 1) % H
      swapped_mask      (query, key) swapped in dk,dv's dropout mask
      no_km_on_dp       km missing on dP;      no_scale_on_dk   scale missing on dK
      rope_forward      rotation applied forward, not inverse;      rope_global   packed rope position taken as the global row"""
    H = case.H
    f = torch.float32
    c32, scale = torch.tensor(_c32(case.scale), dtype=f), torch.tensor(_f32(case.scale), dtype=f)
    qp = q_prime(case.q, case.scale)
    dq, dk, dv = torch.zeros(case.Rq, H * DH, dtype=f), torch.zeros(case.Rk, H * DH, dtype=f), torch.zeros(case.Rk, H * DH, dtype=f)

    def rnd(t):
        return t.to(torch.bfloat16).float()
    for b, h, qs, ks, cl in _blocks(case):
        Q, QP, K, V, DO, OO = (t.float() for t in (case.q[qs, cl], qp[qs, cl], case.k[ks, cl], case.v[ks, cl], case.dO[qs, cl], O_[qs, cl]))
        nq, nk = Q.shape[0], K.shape[0]
        Lr = L[(h + 1) % H if mutate == "wrong_L" else h, qs].float()[:, None]
        delta = (DO * OO).sum(1, keepdim=True)
        km = _km(case, b, h, (nq, nk)).float()
        # ---- dq side
        K0, V0, km0 = K, V, km
        if mutate == "stale_key_tile" and nk > STALE_TILE * 64:
            K0, V0 = K.clone(), V.clone()
            a, n = STALE_TILE * 64, min(64, nk - STALE_TILE * 64)
            K0[a:a + n], V0[a:a + n] = K[a - 256:a - 256 + n], V[a - 256:a - 256 + n]
        if mutate == "unmasked_tail" and nk % 64:
            pad = (-nk) % 64
            K0, V0 = torch.cat([K, K[-1:].expand(pad, DH)]), torch.cat([V, V[-1:].expand(pad, DH)])
            km0 = _km(case, b, h, (nq, nk + pad)).float()
        P = torch.exp2(QP @ K0.T - Lr)
        dP = DO @ V0.T
        x = (dP if mutate == "no_km_on_dp" else dP * km0) - delta
        g = (rnd(x * P) @ K0) * scale
        dq[qs, cl] = g
        # ---- dk,dv side
        Q1, DO1, L1, d1 = Q, DO, Lr, delta
        if mutate == "stale_query_tile" and nq > STALE_TILE * 64:
            Q1, DO1, L1, d1 = Q.clone(), DO.clone(), Lr.clone(), delta.clone()
            a, n = STALE_TILE * 64, min(64, nq - STALE_TILE * 64)
            for dst, src in ((Q1, Q), (DO1, DO), (L1, Lr), (d1, delta)):
                dst[a:a + n] = src[a - 256:a - 256 + n]
        if mutate in ("wrong_record", "wrong_delta") and nq > 64:
            i = torch.arange(nq)
            t, nqt = i // 64, (nq + 63) // 64
            nb = torch.where((t ^ 1) < nqt, t ^ 1, t - 1)
            j = nb * 64 + i % 64
            ok = (j < nq)[:, None]
            j = j.clamp_max(nq - 1)
            d1 = torch.where(ok, delta[j], torch.zeros_like(delta))
            if mutate == "wrong_record":
                L1 = torch.where(ok, Lr[j], torch.full_like(Lr, 1e30))
        km1 = _km(case, b, h, (nq, nk), swapped=mutate == "swapped_mask").float()
        P = torch.exp2((Q1 @ K.T) * c32 - L1)
        dP = DO1 @ V.T
        x = (dP if mutate == "no_km_on_dp" else dP * km1) - d1
        gk = rnd(x * P).T @ Q1
        gk = gk if mutate == "no_scale_on_dk" else gk * scale
        dv[ks, cl] = rnd(P * km1).T @ DO1
        dk[ks, cl] = gk
        if case.cos is not None:
            for buf, rows in ((dq, qs), (dk, ks)):
                t = buf[rows, cl]
                cs, sn = _rope_rows(case, b, rows, t.shape[0], glob=mutate == "rope_global")
                sn = -sn if mutate == "rope_forward" else sn
                lo, hi = _unrope(t[:, :32], t[:, 32:], cs, sn)
                buf[rows, cl] = torch.cat([lo, hi], 1)
    return {"dq": dq, "dk": dk, "dv": dv}


def all_cases():
    """(id, make_case arguments) of every data set the GPU tests use (the layouts they run in share the data)"""
    out = []
    for p in (0.0, 0.1):
        for i, (B, H, Sq, Skv) in enumerate(DENSE + [EXCHANGE]):
            out.append((f"dense_B{B}_H{H}_Sq{Sq}_Skv{Skv}_p{p}", dict(segs=dense_segs(B, Sq, Skv), H=H, seed=300 + 10 * i, p=p)))
        for i, (QL, KL, H) in enumerate(PACKED_CROSS):
            out.append((f"packed_cross{i}_p{p}", dict(segs=packed_segs(QL, KL), H=H, seed=400 + 10 * i, p=p)))
        for i, (QL, H) in enumerate(PACKED_SELF):
            out.append((f"packed_self{i}_p{p}", dict(segs=packed_segs(QL, QL), H=H, seed=500 + 10 * i, p=p, rope=True)))
    return out
