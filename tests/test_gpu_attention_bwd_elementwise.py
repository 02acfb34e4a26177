"""-m gpu: the fused attention backward (csrc/attn64bwd.h: attention_bwd.hip dense, attention_bwd_packed.hip packed) checked
ELEMENTWISE against the fp64 reference and the derived bound of tests/attn_bwd_ref.py, on the row strides the model uses
(ditto_train.hip: q|k|v in one [rows, 3d] buffer with dq|dk|dv likewise; k, v inside the [rows, L*2*d] cross K/V buffer with
dk|dv in [rows, 2d]).  tests/test_attention_bwd_bound.py shows on the CPU that this bound passes the kernels' arithmetic and flags
each bug they can have, on these very data sets.

Every case: inputs carry NaN in everything the kernel must not read (slack rows, 8 pad columns past the last head, the other layer's
K/V columns), outputs start as a bf16-exact sentinel, the workspace has 4 KiB of sentinel behind the byte count passed — all intact
afterwards — and worst_ratio(got, want, e, stored_bf16=True) <= 1.0 on every element of dq, dk and dv.  Each case runs twice: with
the supplied L and O (the backward alone) and with the lse and O the library's own training forward wrote for the same operands."""
import pytest
import torch

import attn_bwd_ref as R
from ditto_tts_amd import hip
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
DH, SLACK, PADC, SENT, WS_TAIL = 64, 96, 8, 1024.0, 4096
NAN = float("nan")


def _buf(rows, width, fill):
    return torch.full((rows + SLACK, width + PADC), fill, dtype=torch.bfloat16, device=DEV)


class _View:
    """columns [col, col + d) of the first `rows` rows of a wider buffer"""

    def __init__(self, buf, col, rows, d):
        self.buf, self.col, self.rows, self.d = buf, col, rows, d

    @property
    def ptr(self):
        return self.buf.data_ptr() + 2 * self.col

    @property
    def ld(self):
        return self.buf.shape[1]

    def put(self, t):
        self.buf[:self.rows, self.col:self.col + self.d] = t.to(DEV)
        return self

    def get(self):
        return self.buf[:self.rows, self.col:self.col + self.d].float().cpu()


def _layout(c, self_layout):
    """device buffers of one case in the model's self- or cross-attention layout: inputs NaN outside the operands, outputs sentinel"""
    d = c.H * DH
    lay = {}
    if self_layout:
        assert c.Rq == c.Rk
        qkv, g = _buf(c.Rq, 3 * d, NAN), _buf(c.Rq, 3 * d, SENT)
        for i, n in enumerate("qkv"):
            lay[n] = _View(qkv, i * d, c.Rq, d).put(getattr(c, n))
            lay["d" + n] = _View(g, i * d, c.Rq, d)
    else:
        kv = _buf(c.Rk, 2 * 2 * d, NAN)   # two layers' K | V: layer 0's columns stay NaN
        lay["q"] = _View(_buf(c.Rq, d, NAN), 0, c.Rq, d).put(c.q)
        lay["k"], lay["v"] = _View(kv, 2 * d, c.Rk, d).put(c.k), _View(kv, 3 * d, c.Rk, d).put(c.v)
        gkv = _buf(c.Rk, 2 * d, SENT)
        lay["dq"] = _View(_buf(c.Rq, d, SENT), 0, c.Rq, d)
        lay["dk"], lay["dv"] = _View(gkv, 0, c.Rk, d), _View(gkv, d, c.Rk, d)
    lay["dO"] = _View(_buf(c.Rq, d, NAN), 0, c.Rq, d).put(c.dO)
    lay["O"] = _View(_buf(c.Rq, d, NAN), 0, c.Rq, d)
    return lay


def _bits(lay, names):
    return {n: lay[n].buf.view(torch.int16).clone() for n in names}


def _guards_intact(lay, names, fill_is_nan=False):
    """everything of the named views' buffers outside the views themselves still holds the fill value"""
    seen = {}
    for n in names:
        v = lay[n]
        m = seen.setdefault(id(v.buf), (v.buf, torch.zeros(v.buf.shape, dtype=torch.bool, device=DEV)))[1]
        m[:v.rows, v.col:v.col + v.d] = True
    for buf, m in seen.values():
        rest = buf[~m].float()
        assert bool(torch.isnan(rest).all() if fill_is_nan else (rest == SENT).all()), f"{names}: written outside the output's own elements"


def _ws(nb):
    return torch.full((nb + WS_TAIL,), 0xA5, dtype=torch.uint8, device=DEV)


class _Dense:
    def __init__(self, B, H, Sq, Skv):
        self.B, self.H, self.Sq, self.Skv = B, H, Sq, Skv
        self.nb = hip.lib().ditto_attention_bwd_workspace_bytes(B, H, Sq, Skv, DH)

    def lse_dev(self, c, L):   # [H, Rq] -> the entry's [B, H, Sq]
        return L.view(self.H, self.B, self.Sq).permute(1, 0, 2).contiguous().to(DEV)

    def forward(self, c, lay):
        lse = torch.full((self.B, self.H, self.Sq), NAN, dtype=torch.float32, device=DEV)
        ws = _ws(self.nb)
        hip.check(hip.lib().ditto_attention_dropout_bf16(lay["q"].ptr, lay["q"].ld, lay["k"].ptr, lay["k"].ld, lay["v"].ptr, lay["v"].ld,
                                                         lay["O"].ptr, lay["O"].ld, lse.data_ptr(), self.B, self.H, self.Sq, self.Skv, DH,
                                                         c.scale, c.p, R.SEED, R.LAYER, ws.data_ptr(), self.nb, stream()))
        torch.cuda.synchronize()
        assert bool((ws[self.nb:] == 0xA5).all()), "the forward wrote behind its workspace"
        return lse.cpu().permute(1, 0, 2).reshape(self.H, c.Rq).contiguous(), lse

    def backward(self, c, lay, lse):
        ws = _ws(self.nb)
        hip.check(hip.lib().ditto_attention_bwd_bf16(
            lay["q"].ptr, lay["q"].ld, lay["k"].ptr, lay["k"].ld, lay["v"].ptr, lay["v"].ld, lay["dO"].ptr, lay["dO"].ld,
            lay["O"].ptr, lay["O"].ld, lse.data_ptr(), lay["dq"].ptr, lay["dq"].ld, lay["dk"].ptr, lay["dk"].ld, lay["dv"].ptr,
            lay["dv"].ld, self.B, self.H, self.Sq, self.Skv, DH, c.scale, c.p, R.SEED, R.LAYER, ws.data_ptr(), self.nb, stream()))
        torch.cuda.synchronize()
        assert bool((ws[self.nb:] == 0xA5).all()), "the backward wrote behind its workspace"


class _Packed:
    """q_rows / kv_rows handed to the entries include the slack rows, so lse [H, q_rows] has slack columns in every head's row"""

    def __init__(self, c, self_attn):
        self.B, self.H, self.self_attn = len(c.segs), c.H, self_attn
        self.RQ, self.RK = c.Rq + SLACK, c.Rk + SLACK
        cu = lambda i: torch.tensor([s[i] for s in c.segs] + [c.segs[-1][i] + c.segs[-1][i + 1]], dtype=torch.int32, device=DEV)  # noqa: E731
        self.cu_q = cu(0)
        self.cu_kv = self.cu_q if self_attn else cu(2)
        self.nb = hip.lib().ditto_attention_bwd_packed_workspace_bytes(self.B, self.H, self.RQ)
        self.cos = self.sin = None
        if c.cos is not None:   # the kernel's tables: one row per position inside the longest utterance
            self.cos, self.sin = c.cos[:c.maxq].contiguous().to(DEV), c.sin[:c.maxq].contiguous().to(DEV)

    def lse_dev(self, c, L):
        out = torch.full((self.H, self.RQ), NAN, dtype=torch.float32, device=DEV)
        out[:, :c.Rq] = L.to(DEV)
        return out

    def forward(self, c, lay):
        lse = torch.full((self.H, self.RQ), NAN, dtype=torch.float32, device=DEV)
        hip.check(hip.lib().ditto_attention_train_packed_bf16(
            lay["q"].ptr, lay["q"].ld, lay["k"].ptr, lay["k"].ld, lay["v"].ptr, lay["v"].ld, lay["O"].ptr, lay["O"].ld, lse.data_ptr(),
            self.cu_q.data_ptr(), self.cu_kv.data_ptr(), self.B, self.H, self.RQ, self.RK, c.maxq, c.maxk, DH, c.scale, c.p, R.SEED,
            R.LAYER, stream()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(lse[:, c.Rq:]).all()), "the forward wrote lse outside every utterance"
        return lse[:, :c.Rq].cpu().contiguous(), lse

    def backward(self, c, lay, lse):
        ws = _ws(self.nb)
        hip.check(hip.lib().ditto_attention_bwd_packed_bf16(
            lay["q"].ptr, lay["q"].ld, lay["k"].ptr, lay["k"].ld, lay["v"].ptr, lay["v"].ld, lay["dO"].ptr, lay["dO"].ld,
            lay["O"].ptr, lay["O"].ld, lse.data_ptr(), lay["dq"].ptr, lay["dq"].ld, lay["dk"].ptr, lay["dk"].ld, lay["dv"].ptr,
            lay["dv"].ld, self.cu_q.data_ptr(), self.cu_kv.data_ptr(), self.B, self.H, self.RQ, self.RK, c.maxq, c.maxk, DH, c.scale,
            c.p, R.SEED, R.LAYER, None if self.cos is None else self.cos.data_ptr(), None if self.sin is None else self.sin.data_ptr(),
            ws.data_ptr(), self.nb, stream()))
        torch.cuda.synchronize()
        assert bool((ws[self.nb:] == 0xA5).all()), "the backward wrote behind its workspace"


def _backward_checked(tag, c, entry, lay, L, lse_dev):
    """one backward on the O now in lay["O"] and the given L: guards, every element within its bound.  Returns the ratios."""
    for n in ("dq", "dk", "dv"):
        lay[n].buf.fill_(SENT)
    ins = ("q", "k", "v", "dO", "O")
    before = _bits(lay, ins)
    lse_before = lse_dev.clone()
    entry.backward(c, lay, lse_dev)
    for n, b in before.items():
        assert torch.equal(lay[n].buf.view(torch.int16), b), f"input {n} was modified"
    assert torch.equal(lse_dev.view(torch.int32), lse_before.view(torch.int32)), "lse was modified"
    _guards_intact(lay, ("dq", "dk", "dv"))
    got = {n: lay[n].get() for n in ("dq", "dk", "dv")}
    O_ = lay["O"].get().to(torch.bfloat16)
    ref = R.reference(c, L, O_)
    r = R.ratios(got, ref)
    # recorded, not asserted: dk / dv against the OTHER definition of P (q' scores throughout), in units of the same bound
    other = R.reference(c, L, O_, qprime_dkdv=True)
    r2 = {n: R.worst_ratio(got[n], getattr(other, n), getattr(ref, "e_" + n), stored_bf16=True) for n in ("dk", "dv")}
    print(f"BWD_RATIO {tag} dq={r['dq']:.3f} dk={r['dk']:.3f} dv={r['dv']:.3f} | q'-scores: dk={r2['dk']:.3f} dv={r2['dv']:.3f}")
    for n, x in r.items():
        assert x <= 1.0, f"{tag}: {n} outside its bound: worst ratio {x:.3f}"
    return r, got


def _both_runs(tag, c, entry, self_layout):
    lay = _layout(c, self_layout)
    lay["O"].put(c.O)
    _backward_checked(tag + " supplied", c, entry, lay, c.L, entry.lse_dev(c, c.L))
    lay["O"].buf.fill_(NAN)
    ins = _bits(lay, ("q", "k", "v"))
    L_fwd, lse_dev = entry.forward(c, lay)
    for n, b in ins.items():
        assert torch.equal(lay[n].buf.view(torch.int16), b), f"the forward modified {n}"
    _guards_intact(lay, ("O",), fill_is_nan=True)
    assert bool(torch.isfinite(L_fwd).all()) and bool(torch.isfinite(lay["O"].get()).all())
    _backward_checked(tag + " forward's", c, entry, lay, L_fwd, lse_dev)


DENSE_RUNS = [(i, s, False) for i, s in enumerate(R.DENSE)] + [(i, s, True) for i, s in enumerate(R.DENSE) if s[2] == s[3]]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("i,shape,self_layout", DENSE_RUNS,
                         ids=["B%d_H%d_Sq%d_Skv%d_%s" % (*s, "self" if sl else "cross") for _, s, sl in DENSE_RUNS])
def test_dense_backward_elementwise(i, shape, self_layout, p):
    B, H, Sq, Skv = shape
    c = R.make_case(R.dense_segs(B, Sq, Skv), H, seed=300 + 10 * i, p=p)
    _both_runs(f"dense {shape} {'self' if self_layout else 'cross'} p={p}", c, _Dense(B, H, Sq, Skv), self_layout)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("i", range(len(R.PACKED_CROSS)))
def test_packed_backward_elementwise_cross_layout(i, p):
    QL, KL, H = R.PACKED_CROSS[i]
    c = R.make_case(R.packed_segs(QL, KL), H, seed=400 + 10 * i, p=p)
    _both_runs(f"packed cross {QL} x {KL} p={p}", c, _Packed(c, False), False)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("i", range(len(R.PACKED_SELF)))
def test_packed_backward_elementwise_self_layout_with_fused_inverse_rotation(i, p):
    QL, H = R.PACKED_SELF[i]
    c = R.make_case(R.packed_segs(QL, QL), H, seed=500 + 10 * i, p=p, rope=True)
    _both_runs(f"packed self+rope {QL} p={p}", c, _Packed(c, True), True)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dense_backward_takes_each_heads_own_L(p):
    """The supplied L and O, then L of the two heads exchanged: the outputs must match the reference built from the exchanged L (and so
    differ from the first run's), which pins L to the right head whatever symmetry the data have."""
    B, H, Sq, Skv = R.EXCHANGE
    c = R.make_case(R.dense_segs(B, Sq, Skv), H, seed=300 + 10 * len(R.DENSE), p=p)
    entry = _Dense(B, H, Sq, Skv)
    lay = _layout(c, True)
    lay["O"].put(c.O)
    _, got = _backward_checked(f"dense {R.EXCHANGE} self p={p} supplied", c, entry, lay, c.L, entry.lse_dev(c, c.L))
    L2 = c.L.flip(0).contiguous()
    _, got2 = _backward_checked(f"dense {R.EXCHANGE} self p={p} L exchanged", c, entry, lay, L2, entry.lse_dev(c, L2))
    for n in got:
        assert not torch.equal(got[n], got2[n])
