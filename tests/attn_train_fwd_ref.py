"""The training attention forward's fp64 reference, an elementwise error bound derived from the kernel's arithmetic, and a CPU model of
that arithmetic with the bugs the bound must catch (plain helpers, shared by test_attention_train_fwd_bound.py,
test_gpu_attention_train_fwd_elementwise.py and the two forward / backward vs autograd tests; the data sets, q', the keep mask and the
block iteration are attn_bwd_ref.py's, U, G and worst_ratio attn_ref.py's).

The forward (csrc/attn64v2.h, TRAIN / DROP: attention_train.hip dense, attention_train_packed.hip packed) is a function of
(q, k, v, scale, p, seed, layer) and, in the residual forms, of the stream.  Per (utterance, head), with c = fp32(scale) * fp32(log2 e)
and km = keep mask / (1 - p) (1 without dropout):

    q' = bf16(fp32(q) c)      S = q'.k      L = log2 sum_j 2^S_ij      W = 2^(S - L)      O = (W km) V
    plain: out = bf16(O), lse = L       residual: stream_out = stream_in + O (fp32, or one bf16 store), O beside it as bf16 when asked

The row sum is the FULL softmax's: km applies to the P V operand only.  The kernel keeps a running maximum m_run that is an octave
ceiling with a deferred raise (ATT_RESCALE_THR_LOG2 = 8): ceil(tile 0's maximum), raised to ceil(...) only when a row exceeds it by more
than 8, so m_run lies within 9 of the true row maximum and e_ij = exp2(S_ij - m_run) <= 2^9.  attn_flags 8192 routes the dense forms to
the older attn64_kernel<.., TRAIN>, whose scores are c (q.k) on the RAW q: reference(raw_q=True) follows that definition.

THE BOUND, term by term (u = U = 2^-8 bf16 roundoff, G = 2^-24; every fp32 sum of the matrix pipe is charged 2 G per term: its
internal rounding is not documented as round-to-nearest):
  score   64 fp32 products and the -m_run start of the MFMA chain (older kernel: 64 products, the factor c and the subtraction):
          |ds_ij| <= 2 G (dh + 2) a_ij,  a_ij = sum_c |q'_ic k_jc| (log2 units) + |m_run|,  |m_run| <= |max_j S_ij| + 9.
  exp     v_exp_f32: EXP = 2^-22 relative (one ulp of the documented accuracy, doubled).
          => e_ij is off by rho_ij = ln2 |ds_ij| + EXP, relatively.
  P V     operand bf16(e km): the product in fp32, one bf16 rounding: rho + u + 2 G per weight.
  row sum l = sum_j bf16(e_ij) through the all-ones MFMA, n = the tile-padded key count terms in fp32.  Relative to the true sum
          dl_i = sum_j W_ij (rho_ij + u) + 2 G (n + 8): the weights are the full softmax's, not the masked ones.
  O       the numerator N = sum_j bf16(e km) v in fp32 over n terms, then one product with 1 / l (a reciprocal and a product: 4 G):
          |O_hat - O| <= sum_j W km (rho + u + 2 G) |v| + 2 G (n + 8) sum_j W km |v|
                         + (that first sum + sum_j W km |v|) dl (1 + 2 dl) + 4 G |O|
          fp32 stream: + 2 G |want| (one fp32 add).  bf16 stream: the add happens in fp32 before ONE bf16 store, so the same bound
          with worst_ratio(stored_bf16=True).  O beside the stream, and the plain form's out: the bound of O with one bf16 store.
  lse     L_hat = m_run + log2(l_hat):  |L_hat - L| <= dl (1 + dl) / ln2 + (LOG + 2 G) (|L| + |m_run|), LOG = 2^-22 for v_log_f32 (one
          ulp, doubled) and 2 G for the fp32 subtraction, both taken at the magnitude |L| + |m_run| that bounds every operand.
No element is excluded.  On every data set of all_cases() the lse bound stays at or below 2^-7 log2 units (u / ln2 dominates: at most
6.5e-3), which test_attention_train_fwd_bound.py asserts.  A row whose every key is dropped has W km = 0: the bound is 0 there, so O
must be exactly 0 (and the fp32 stream exactly its input)."""
import math
from types import SimpleNamespace

import torch

from attn_bwd_ref import (DENSE, EXCHANGE, LAYER, PACKED_CROSS, PACKED_SELF, SEED, _blocks, _c32, _km, all_cases,  # noqa: F401
                          dense_segs, keep_scale, make_case, packed_segs, q_prime)
from attn_ref import G, U, worst_ratio   # noqa: F401  (re-exported for the tests)
from gpu_util import asym
from oracle import ditto_oracle as O

DH = 64
EXP = 2.0 ** -22
LOG = 2.0 ** -22
M_SLACK = 9.0          # |m_run - true row maximum| <= 9: an octave ceiling (1) and the deferred raise (8)
LN2 = math.log(2.0)
STALE_TILE = 5         # a key tile whose buffer's previous occupant in the two-buffer ring (tile 3) exists and is a whole tile
OUT_INIT = 1024.0      # what the GPU test's output buffers hold before the launch (resid_from_out reads it)
BF16_STORED = {"O": True, "L": False, "stream_f32": False, "stream_bf16": True, "beside": True}


def build(cid, kw):
    """the data set `cid` of all_cases(): make_case(**kw), marked packed by its id (the packed-only mutation looks at it)"""
    c = make_case(**kw)
    c.packed = cid.startswith("packed")
    return c


def make_resid(case, seed=77):
    """the stream's input rows [Rq, H * 64] as bf16-exact fp32 (usable on either stream), large against O so that a difference of two
    bf16 stream rows is visibly not O"""
    return (asym((case.Rq, case.H * DH), seed) * 8.0).to(torch.bfloat16).float()


def reference(case, resid=None, raw_q=False):
    """fp64 on the exact operands: O [Rq, H * 64] UNROUNDED, L [H, Rq], the elementwise bounds e_O (before any store) and e_L (module
    docstring), stream = resid + O with e_stream (the fp32 add included) when resid is given.  raw_q: scores c (q.k) on the raw q (the
    older kernel).  Only case.q / k / v / segs / H / scale / p / keep are read."""
    H, c32 = case.H, _c32(case.scale)
    Rq = case.q.shape[0]
    r = SimpleNamespace(O=torch.zeros(Rq, H * DH, dtype=torch.float64), L=torch.zeros(H, Rq, dtype=torch.float64))
    r.e_O, r.e_L = torch.zeros_like(r.O), torch.zeros_like(r.L)
    qp = q_prime(case.q, case.scale)
    for b, h, qs, ks, cl in _blocks(case):
        K, V = case.k[ks, cl].double(), case.v[ks, cl].double()
        if raw_q:
            Q = case.q[qs, cl].double()
            S, a = c32 * (Q @ K.T), c32 * (Q.abs() @ K.abs().T)
        else:
            Q = qp[qs, cl].double()
            S, a = Q @ K.T, Q.abs() @ K.abs().T
        nq, nk = S.shape
        n = 64 * ((nk + 63) // 64)
        mx = S.amax(1, keepdim=True)
        m_abs = mx.abs() + M_SLACK
        L = mx + torch.log2(torch.exp2(S - mx).sum(1, keepdim=True))
        W = torch.exp2(S - L)
        rho = LN2 * 2 * G * (DH + 2) * (a + m_abs) + EXP
        dl = (W * (rho + U)).sum(1, keepdim=True) + 2 * G * (n + 8)
        Wk = W * _km(case, b, h, (nq, nk))
        o, A = Wk @ V, Wk @ V.abs()
        t1 = (Wk * (rho + U + 2 * G)) @ V.abs()
        r.O[qs, cl] = o
        r.e_O[qs, cl] = t1 + 2 * G * (n + 8) * A + (t1 + A) * dl * (1 + 2 * dl) + 4 * G * o.abs() + 1e-30
        r.L[h, qs] = L[:, 0]
        r.e_L[h, qs] = (dl * (1 + dl) / LN2 + (LOG + 2 * G) * (L.abs() + m_abs))[:, 0]
    if resid is not None:
        r.stream = resid.double() + r.O
        r.e_stream = r.e_O + 2 * G * r.stream.abs()
    return r


def bound(ref):
    """{form: (want, e)} of a reference(): plain O / O beside, lse, and the two streams when the reference has a residual"""
    out = {"O": (ref.O, ref.e_O), "beside": (ref.O, ref.e_O), "L": (ref.L, ref.e_L)}
    if hasattr(ref, "stream"):
        out["stream_f32"] = out["stream_bf16"] = (ref.stream, ref.e_stream)
    return out


def ratios(got, ref, stored=True):
    """worst ratio of each form present in got against bound(ref).  stored: the bf16 outputs are as stored (half an ulp granted)"""
    b = bound(ref)
    return {n: worst_ratio(t, *b[n], stored_bf16=stored and BF16_STORED[n]) for n, t in got.items()}


def _differs(case, other):
    return any(not torch.equal(_km(case, b, h, (s[1], s[3])), other(b, h, s)) for b, s in enumerate(case.segs) for h in range(case.H))


def _other_head_km(case, b, h, shape):
    bh = (b * case.H + h + 1) % (len(case.segs) * case.H)
    return _km(case, bh // case.H, bh % case.H, shape)


def _global_km(case, b, h, q0, shape):
    """the mask taken at the GLOBAL query row of a packed batch (the bug); generated here: make_case's square covers local rows only"""
    nq, nk = shape
    if not hasattr(case, "_keep_glob"):
        case._keep_glob = O.hash_dropout_mask(SEED, LAYER, len(case.segs), case.H, case.Rq, case.maxk, case.p)
    return case._keep_glob[b, h, q0:q0 + nq, :nk].double() * keep_scale(case.p)


def mutations(case):
    """the bugs of emulate() that exist at this case (one of the outputs must leave its bound); raw_q_scores is recorded, not listed"""
    nkt = max((s[3] + 63) // 64 for s in case.segs)
    B = len(case.segs)
    m = ["ln_not_log2", "resid_dropped", "resid_from_out", "o_beside_is_delta"]
    if nkt > STALE_TILE:
        m.append("stale_key_tile")
    if any(s[3] % 64 for s in case.segs):
        m.append("unmasked_tail")
    if case.H > 1:
        m.append("lse_head_swap")
    if B > 1:
        m.append("lse_wrong_slot")
    if case.p > 0:
        m += ["no_keep_scale", "masked_rowsum"]
        # (on a block this small two masks can coincide; the mutation is then the identity)
        if _differs(case, lambda b, h, s: _km(case, b, h, (s[1], s[3]), swapped=True)):
            m.append("swapped_mask")
        if B * case.H > 1 and _differs(case, lambda b, h, s: _other_head_km(case, b, h, (s[1], s[3]))):
            m.append("other_head_mask")
        if getattr(case, "packed", False) and _differs(case, lambda b, h, s: _global_km(case, b, h, s[0], (s[1], s[3]))):
            m.append("packed_global_mask")
    return m


def emulate(case, resid=None, mutate=None, raw_q=False):
    """A CPU model of the kernel's arithmetic: bf16 q', fp32 scores, m = ceil(row max), pl = bf16(exp2(S - m)), pv = bf16(exp2(S - m) km),
    l = sum pl in fp32, O = (pv V) / l, L = m + log2 l, the residual add — every result in fp32 BEFORE its store (the tests round) —
    and the bugs the bound must catch:
      unmasked_tail       the clamped copies of the last key in a ragged last tile counted
      stale_key_tile      key tile 5 taken from the two-buffer ring's previous occupant (tile 3)
      swapped_mask        the mask indexed (key, query);      other_head_mask   the mask of stream b H + h + 1
      packed_global_mask  packed: the mask taken at the global query row, not the utterance-local one
      no_keep_scale       1 / (1 - p) missing;      masked_rowsum   l summed from the masked probabilities
      ln_not_log2         lse written in the natural-log domain
      lse_head_swap       lse of head (h + 1) % H;      lse_wrong_slot   lse written at the next utterance's slots (the rest stays NaN)
      raw_q_scores        scores c (q.k) on the raw q (the other definition: recorded by the tests, not asserted)
      resid_dropped       the stream written without its input;      resid_from_out   the input read from the output buffer, out of place
      o_beside_is_delta   O beside the bf16 stream written as stream_after - stream_before of the two bf16 rows
    Returns {O, L} and, with resid, {stream_f32, stream_bf16, beside}."""
    H, f = case.H, torch.float32
    Rq = case.q.shape[0]
    c32 = torch.tensor(_c32(case.scale), dtype=f)
    qp = q_prime(case.q, case.scale)
    o_all = torch.zeros(Rq, H * DH, dtype=f)
    L_all = torch.full((H, Rq), float("nan"), dtype=f)
    B = len(case.segs)

    def rnd(t):
        return t.to(torch.bfloat16).float()
    for b, h, qs, ks, cl in _blocks(case):
        K, V = case.k[ks, cl].float(), case.v[ks, cl].float()
        nq, nk = qs.stop - qs.start, K.shape[0]
        if mutate == "swapped_mask":
            km = _km(case, b, h, (nq, nk), swapped=True)
        elif mutate == "other_head_mask":
            km = _other_head_km(case, b, h, (nq, nk))
        elif mutate == "packed_global_mask":
            km = _global_km(case, b, h, qs.start, (nq, nk))
        else:
            km = _km(case, b, h, (nq, nk))
        if mutate == "no_keep_scale":
            km = (km > 0).double()
        if mutate == "stale_key_tile" and nk > STALE_TILE * 64:
            K, V = K.clone(), V.clone()
            a, n = STALE_TILE * 64, min(64, nk - STALE_TILE * 64)
            K[a:a + n], V[a:a + n] = K[a - 128:a - 128 + n].clone(), V[a - 128:a - 128 + n].clone()
        if mutate == "unmasked_tail" and nk % 64:
            pad = (-nk) % 64
            K, V = torch.cat([K, K[-1:].expand(pad, DH)]), torch.cat([V, V[-1:].expand(pad, DH)])
            km = _km(case, b, h, (nq, nk + pad))
        km = km.float()
        if raw_q or mutate == "raw_q_scores":
            S = (case.q[qs, cl].float() @ K.T) * c32
        else:
            S = qp[qs, cl].float() @ K.T
        m = torch.ceil(S.amax(1, keepdim=True))
        e = torch.exp2(S - m)
        pl, pv = rnd(e), rnd(e * km)
        l = (pv if mutate == "masked_rowsum" else pl).sum(1, keepdim=True)
        o_all[qs, cl] = (pv @ V) * (1.0 / l)
        L = (m + torch.log2(l))[:, 0]
        if mutate == "ln_not_log2":
            L = L * LN2
        hd = (h + 1) % H if mutate == "lse_head_swap" else h
        if mutate == "lse_wrong_slot":
            q0 = case.segs[(b + 1) % B][0]
            nw = min(nq, Rq - q0)
            L_all[hd, q0:q0 + nw] = L[:nw]
        else:
            L_all[hd, qs] = L
    out = {"O": o_all, "L": L_all}
    if resid is not None:
        rin = torch.zeros_like(resid) if mutate == "resid_dropped" else torch.full_like(resid, OUT_INIT) if mutate == "resid_from_out" \
            else resid.float()
        out["stream_f32"] = out["stream_bf16"] = rin + o_all
        out["beside"] = rnd(out["stream_bf16"]) - rnd(resid) if mutate == "o_beside_is_delta" else o_all
    return out
