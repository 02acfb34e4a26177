"""-m gpu: the training attention forward (csrc/attn64v2.h TRAIN / DROP: attention_train.hip dense, attention_train_packed.hip packed)
checked ELEMENTWISE against the fp64 reference and the derived bound of tests/attn_train_fwd_ref.py: O, the log-sum-exp, and the
residual forms (fp32 stream in and out of place, bf16 stream with O beside it, packed fp32 stream with O in its own slot) through
ditto_attention_train_resid_bf16, on the row strides the model uses (q|k|v in one [rows, 3d] buffer; k, v inside the [rows, L*2*d] cross
K/V buffer with the other layer's columns NaN; the bf16 stream [M, d] followed directly by O [M, d]).
tests/test_attention_train_fwd_bound.py shows on the CPU that this bound passes the kernel's arithmetic and flags each bug it can have,
on these very data sets.

Every case: inputs carry NaN in everything the kernel must not read (slack rows, 8 pad columns, rows outside every utterance), outputs
and lse start as sentinels and everything outside their own elements is intact afterwards, inputs are bitwise unchanged, two runs are
bitwise equal, worst_ratio <= 1.0 on every element of every output and max |L_hat - L| / e_L <= 1.0.  One FWD_RATIO line per case.
The threshold is the derived 1.0; the worst ratios measured on an MI355X are recorded here, not turned into thresholds:
    attn64v2 TRAIN / DROP, dense and packed, all forms:  O / stream / O beside 0.635 (p = 0.1; 0.352 at p = 0),  lse 0.858
    attn_flags 8192 (attn64_kernel<.., TRAIN>):          O / stream 0.426,  lse 0.001 (its row sum is the fp32 sum of unrounded terms)
which is what the CPU model of test_attention_train_fwd_bound.py gives on the same data (0.62 and 0.86)."""
import functools
import math

import pytest
import torch

import attn_train_fwd_ref as R
from ditto_tts_amd import hip
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
DH, SLACK, PADC, SENT, LSE_TAIL = 64, 96, 8, 1024.0, 64
NAN = float("nan")
ENTRY = "ditto_attention_train_resid_bf16"
CASES = dict(R.all_cases())
DENSE_FORMS = ("plain", "resid_f32_inplace", "resid_f32_outofplace", "resid_bf16_beside")
PACKED_FORMS = DENSE_FORMS + ("resid_f32_oslot",)


@functools.lru_cache(maxsize=None)
def _data(cid):
    """the data set, its stream input and the fp64 reference with its bounds: computed on the CPU once, shared, never modified"""
    c = R.build(cid, CASES[cid])
    resid = R.make_resid(c)
    return c, resid, R.reference(c, resid)


@functools.lru_cache(maxsize=None)
def _raw_reference(cid):
    c, resid, _ = _data(cid)
    return R.reference(c, resid, raw_q=True)


class _View:
    """columns [col, col + d) of rows [row0, row0 + rows) of a wider 2-D buffer"""

    def __init__(self, buf, col, rows, d, row0=0, nbytes=None):
        self.buf, self.col, self.rows, self.d, self.row0 = buf, col, rows, d, row0
        self.esz = buf.element_size()
        self.off = (row0 * buf.shape[1] + col) * self.esz
        self.nbytes = buf.numel() * self.esz - self.off if nbytes is None else nbytes

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    @property
    def ld(self):
        return self.buf.shape[1]

    def put(self, t):
        self.buf[self.row0:self.row0 + self.rows, self.col:self.col + self.d] = t.to(self.buf.dtype).to(DEV)
        return self

    def get(self):
        return self.buf[self.row0:self.row0 + self.rows, self.col:self.col + self.d].float().cpu()

    def sub(self, r0, n):
        return _View(self.buf, self.col, n, self.d, self.row0 + r0)


def _buf(rows, width, fill, dtype=torch.bfloat16, pad=PADC):
    return torch.full((rows + SLACK, width + pad), fill, dtype=dtype, device=DEV)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


def _inputs(c, self_layout):
    """q, k, v of one case in the model's self- or cross-attention layout, NaN outside the operands"""
    d = c.H * DH
    if self_layout:
        assert c.Rq == c.Rk
        qkv = _buf(c.Rq, 3 * d, NAN)
        return {n: _View(qkv, i * d, c.Rq, d).put(getattr(c, n)) for i, n in enumerate("qkv")}
    kv = _buf(c.Rk, 2 * 2 * d, NAN)   # two layers' K | V: layer 0's columns stay NaN
    return {"q": _View(_buf(c.Rq, d, NAN), 0, c.Rq, d).put(c.q), "k": _View(kv, 2 * d, c.Rk, d).put(c.k),
            "v": _View(kv, 3 * d, c.Rk, d).put(c.v)}


class _Geo:
    """one launch's geometry.  Dense: B utterances of Sq x Skv.  Packed: q_rows / kv_rows handed to the entries include the slack rows,
    so lse [H, q_rows] has slack columns in every head's row"""

    def __init__(self, H, segs=None, dense=None):
        self.H, self.packed = H, dense is None
        if self.packed:
            self.B, self.segs = len(segs), segs
            self.Rq, self.Rk = segs[-1][0] + segs[-1][1], segs[-1][2] + segs[-1][3]
            self.Sq, self.Skv = self.Rq + SLACK, self.Rk + SLACK
            self.max_q, self.max_kv = max(s[1] for s in segs), max(s[3] for s in segs)
            cu = lambda i: torch.tensor([s[i] for s in segs] + [segs[-1][i] + segs[-1][i + 1]], dtype=torch.int32, device=DEV)  # noqa: E731
            self.cu_q, self.cu_kv = cu(0), cu(2)
            self.lse_shape = (H, self.Sq)
        else:
            self.B, self.Sq, self.Skv = dense
            self.max_q, self.max_kv, self.Rq, self.Rk = self.Sq, self.Skv, self.B * self.Sq, self.B * self.Skv
            self.cu_q = self.cu_kv = None
            self.lse_shape = (self.B, H, self.Sq)

    def lse_rows(self, lse):
        """the valid slots as [H, Rq] on the CPU, and a mask of them over the device buffer (with its tail)"""
        n = math.prod(self.lse_shape)
        body, valid = lse[:n].view(self.lse_shape), torch.zeros(lse.numel(), dtype=torch.bool, device=DEV)
        if self.packed:
            valid[:n].view(self.lse_shape)[:, :self.Rq] = True
            return body[:, :self.Rq].cpu().contiguous(), valid
        valid[:n] = True
        return body.cpu().permute(1, 0, 2).reshape(self.H, self.Rq).contiguous(), valid


def _geo(c, cid):
    if cid.startswith("packed"):
        return _Geo(c.H, segs=c.segs)
    return _Geo(c.H, dense=(len(c.segs), c.segs[0][1], c.segs[0][3]))


def _execute(scale, geo, ins, form, p, resid, flags=3):
    """one launch of `form` with fresh outputs: guards, inputs unchanged.  Returns {output name: fp32 CPU tensor [Rq, d]} and L [H, Rq]."""
    lib = hip.lib()
    d, Rq = geo.H * DH, geo.Rq
    M = geo.Sq if geo.packed else Rq             # the rows the model's buffers hold
    n_lse = math.prod(geo.lse_shape)
    lse = torch.full((n_lse + LSE_TAIL,), SENT, dtype=torch.float32, device=DEV)
    rin = rout = o = None
    if form == "plain" or form == "resid_f32_oslot":
        o = _View(_buf(Rq, d, SENT), 0, Rq, d)
    if form == "resid_f32_inplace":
        rout = _View(_buf(Rq, d, SENT, torch.float32), 0, Rq, d).put(resid)
    elif form in ("resid_f32_outofplace", "resid_f32_oslot"):
        rin = _View(_buf(Rq, d, NAN, torch.float32), 0, Rq, d).put(resid)
        rout = _View(_buf(Rq, d, SENT, torch.float32), 0, Rq, d)
    elif form == "resid_bf16_beside":              # as the model lays it out: the bf16 stream [M, d], then O [M, d], no pad columns
        rin = _View(_buf(Rq, d, NAN, pad=0), 0, Rq, d).put(resid)   # (one ldr serves both streams)
        both = torch.full((2 * M + SLACK, d), SENT, dtype=torch.bfloat16, device=DEV)
        rout, o = _View(both, 0, Rq, d, 0, nbytes=M * d * 2), _View(both, 0, Rq, d, M)
    watched = [v for v in (ins["q"], ins["k"], ins["v"], rin) if v is not None]
    before = [(v, _bits(v.buf)) for v in watched]
    stream_before = None if form != "resid_f32_inplace" else rout.get()
    try:
        hip.set_option("attn_flags", flags)
        if form == "plain" and geo.packed:
            rc = lib.ditto_attention_train_packed_bf16(
                ins["q"].ptr, ins["q"].ld, ins["k"].ptr, ins["k"].ld, ins["v"].ptr, ins["v"].ld, o.ptr, o.ld, lse.data_ptr(),
                geo.cu_q.data_ptr(), geo.cu_kv.data_ptr(), geo.B, geo.H, geo.Sq, geo.Skv, geo.max_q, geo.max_kv, DH, scale, p, R.SEED,
                R.LAYER, stream())
        elif form == "plain":
            nb = lib.ditto_attention_bwd_workspace_bytes(geo.B, geo.H, geo.Sq, geo.Skv, DH)
            ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
            rc = lib.ditto_attention_dropout_bf16(ins["q"].ptr, ins["q"].ld, ins["k"].ptr, ins["k"].ld, ins["v"].ptr, ins["v"].ld, o.ptr,
                                                  o.ld, lse.data_ptr(), geo.B, geo.H, geo.Sq, geo.Skv, DH, scale, p, R.SEED, R.LAYER,
                                                  ws.data_ptr(), nb, stream())
        else:
            rc = hip.call(ENTRY, **_entry_args(geo, ins, rin, rout, o, lse, scale, p))
        hip.check(rc)
        torch.cuda.synchronize()
    finally:
        hip.set_option("attn_flags", 3)
    if form == "plain" and not geo.packed:
        assert bool((ws[nb:] == 0xA5).all()), "the forward wrote behind its workspace"
    for v, b in before:
        assert torch.equal(_bits(v.buf), b), "an input was modified"
    outs = [v for v in (rout, o) if v is not None]
    seen = {}
    for v in outs:
        m = seen.setdefault(id(v.buf), (v.buf, torch.zeros(v.buf.shape, dtype=torch.bool, device=DEV)))[1]
        m[v.row0:v.row0 + v.rows, v.col:v.col + v.d] = True
    for buf, m in seen.values():
        assert bool((buf[~m].float() == SENT).all()), f"{form}: written outside the output's own elements"
    L, valid = geo.lse_rows(lse)
    assert bool((lse[~valid] == SENT).all()), f"{form}: lse written outside the valid slots"
    got = {"L": L}
    if form == "plain":
        got["O"] = o.get()
    else:
        got["stream_bf16" if form == "resid_bf16_beside" else "stream_f32"] = rout.get()
        if o is not None:
            got["beside"] = o.get()
    return got, stream_before


def _entry_args(geo, ins, rin, rout, o, lse, scale, p, **over):
    kw = dict(q=ins["q"].ptr, q_bytes=ins["q"].nbytes, ldq=ins["q"].ld, k=ins["k"].ptr, k_bytes=ins["k"].nbytes, ldk=ins["k"].ld,
              v=ins["v"].ptr, v_bytes=ins["v"].nbytes, ldv=ins["v"].ld,
              resid_in=None if rin is None else rin.ptr, resid_in_bytes=0 if rin is None else rin.nbytes,
              resid_out=rout.ptr, resid_out_bytes=rout.nbytes, ldr=rout.ld, resid_bf16=int(rout.esz == 2),
              out=None if o is None else o.ptr, out_bytes=0 if o is None else o.nbytes, ldo=0 if o is None else o.ld,
              lse_out=lse.data_ptr(), lse_out_bytes=lse.numel() * 4,
              cu_q=None if geo.cu_q is None else geo.cu_q.data_ptr(), cu_q_bytes=0 if geo.cu_q is None else geo.cu_q.numel() * 4,
              cu_kv=None if geo.cu_kv is None else geo.cu_kv.data_ptr(), cu_kv_bytes=0 if geo.cu_kv is None else geo.cu_kv.numel() * 4,
              B=geo.B, H=geo.H, Sq=geo.Sq, Skv=geo.Skv, max_q=geo.max_q, max_kv=geo.max_kv, dh=DH, scale=scale, dropout_p=p, seed=R.SEED,
              layer=R.LAYER, stream=stream())
    kw.update(over)
    return kw


def _same(a, b):
    return all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in a) and set(a) == set(b)


def _value(got):
    """the output that carries O: plain O, or the stream"""
    return got["O"] if "O" in got else got.get("stream_f32", got.get("stream_bf16"))


def _dropped_rows(c):
    """bool [Rq, H]: rows of a head whose every key is dropped"""
    out = torch.zeros(c.Rq, c.H, dtype=torch.bool)
    if c.keep is not None:
        for b, h, qs, ks, cl in R._blocks(c):
            out[qs, h] = R._km(c, b, h, (qs.stop - qs.start, ks.stop - ks.start)).sum(1) == 0
    return out


def _checked(tag, c, ref, got, form, resid, stream_before=None):
    r = R.ratios(got, ref)
    print(f"FWD_RATIO {tag} O={max(x for n, x in r.items() if n != 'L'):.3f} L={r['L']:.3f}", {n: round(x, 3) for n, x in r.items()})
    for n, x in r.items():
        assert x <= 1.0, f"{tag}: {n} outside its bound: worst ratio {x:.3f}"
    dropped = _dropped_rows(c).repeat_interleave(DH, dim=1)
    if bool(dropped.any()):
        if form == "plain":
            assert bool((got["O"][dropped] == 0).all()), f"{tag}: a row whose every key is dropped is not exactly 0"
        elif "stream_f32" in got:
            assert torch.equal(got["stream_f32"][dropped], resid[dropped]), f"{tag}: an all-dropped row is not exactly the residual"
    if stream_before is not None:
        assert torch.equal(stream_before, resid)
    return r


def _runs():
    out = []
    for cid in CASES:
        segs = CASES[cid]["segs"]
        packed = cid.startswith("packed")
        self_ok = all(s[0] == s[2] and s[1] == s[3] for s in segs)
        layouts = [True] if cid.startswith("packed_self") else [False, True] if self_ok and not packed else [False]
        for sl in layouts:
            out += [(cid, sl, f) for f in (PACKED_FORMS if packed else DENSE_FORMS)]
    return out


RUNS = _runs()


def instantiation(packed, form, p, flags=3):
    """launch_attention's route for a training forward (lse_out set), restated: the layout picks the translation unit, a residual
    pointer RESID, a non-zero dropout threshold DROP; attn_flags 8192 takes the dense forms to the older kernel"""
    if flags & 8192:
        assert not packed and form in ("plain", "resid_f32_inplace", "resid_f32_outofplace")
        return ("attn64_kernel", form != "plain", None)
    return ("attn64v2 packed" if packed else "attn64v2 dense", form != "plain", p > 0)


def test_every_train_instantiation_is_launched_by_some_case():
    """the eight TRAIN instantiations (RESID x DROP, dense and packed) are each reached by a kernel-level case of RUNS"""
    reached = {instantiation(cid.startswith("packed"), form, CASES[cid]["p"]) for cid, _, form in RUNS}
    assert reached == {(lay, resid, drop) for lay in ("attn64v2 dense", "attn64v2 packed") for resid in (False, True) for drop in (False, True)}
    assert {f for _, _, f in RUNS} == set(PACKED_FORMS)


@pytest.mark.parametrize("cid,self_layout,form", RUNS, ids=[f"{c}-{'self' if s else 'cross'}-{f}" for c, s, f in RUNS])
def test_forward_elementwise(cid, self_layout, form):
    c, resid, ref = _data(cid)
    geo = _geo(c, cid)
    ins = _inputs(c, self_layout)
    tag = f"{cid} {'self' if self_layout else 'cross'} {form}"
    got, before = _execute(c.scale, geo, ins, form, c.p, resid)
    _checked(tag, c, ref, got, form, resid, before)
    again, _ = _execute(c.scale, geo, ins, form, c.p, resid)
    assert _same(got, again), f"{tag}: two runs differ"
    if c.p > 0:   # dropout does something: the same launch without it gives another O
        plain0, _ = _execute(c.scale, geo, ins, form, 0.0, resid)
        assert not torch.equal(_value(plain0), _value(got)), f"{tag}: p = {c.p} changed no element"
    if geo.packed and form in ("plain", "resid_f32_outofplace"):
        # each utterance's packed result is bitwise the dense entry's on that utterance alone: the same body, an utterance-local mask.
        # The mask's stream is b H + h, which a dense launch of one utterance can only give for b = 0: with dropout, that one.
        for b, (q0, nq, k0, nk) in enumerate(c.segs if c.p == 0 else c.segs[:1]):
            sub = {"q": ins["q"].sub(q0, nq), "k": ins["k"].sub(k0, nk), "v": ins["v"].sub(k0, nk)}
            alone, _ = _execute(c.scale, _Geo(c.H, dense=(1, nq, nk)), sub, form, c.p, resid[q0:q0 + nq])
            for n, t in alone.items():
                mine = got[n][:, q0:q0 + nq] if n == "L" else got[n][q0:q0 + nq]
                assert torch.equal(mine.view(torch.int32), t.view(torch.int32)), f"{tag}: utterance {b} differs from the dense entry's {n}"


def test_lse_goes_to_each_heads_own_slot():
    """EXCHANGE, H = 2: lse of head 0 and head 1 each match their own reference (above) and differ from each other's"""
    cid = next(c for c in CASES if "Sq130_Skv130_p0.0" in c)
    c, resid, ref = _data(cid)
    assert c.H == 2
    for form in ("plain", "resid_f32_outofplace"):
        got, _ = _execute(c.scale, _geo(c, cid), _inputs(c, True), form, c.p, resid)
        for h in range(2):
            assert R.worst_ratio(got["L"][h], ref.L[h], ref.e_L[h]) <= 1.0
            assert R.worst_ratio(got["L"][h], ref.L[1 - h], ref.e_L[1 - h]) > 2.0


def test_all_dropped_rows_exist_in_the_data():
    """some data set has rows whose every key is dropped (a single key, p = 0.1), so the exact-zero / exact-residual check runs"""
    assert any(bool(_dropped_rows(_data(cid)[0]).any()) for cid in CASES if CASES[cid]["p"] > 0)


OLD_RUNS = [(cid, f) for cid in CASES if not cid.startswith("packed") for f in ("plain", "resid_f32_inplace", "resid_f32_outofplace")]


@pytest.mark.parametrize("cid,form", OLD_RUNS, ids=[f"{c}-{f}" for c, f in OLD_RUNS])
def test_older_kernel_route_elementwise(cid, form):
    """attn_flags 8192, the A/B route to attn64_kernel<.., TRAIN>: its scores are c (q.k) on the raw q, so its reference is built from
    that definition (reference(raw_q=True)); same bound, same guards.  The flag is restored in _execute's finally."""
    c, resid, _ = _data(cid)
    assert instantiation(False, form, c.p, 8192)[0] == "attn64_kernel"
    got, before = _execute(c.scale, _geo(c, cid), _inputs(c, False), form, c.p, resid, flags=8192)
    assert hip.get_option("attn_flags") == 3
    _checked(f"{cid} attn_flags=8192 {form}", c, _raw_reference(cid), got, form, resid, before)


def test_refusals_are_answered_before_launch():
    """a short buffer, a stride that is no multiple of 8, head_dim 128, a null lse_out, the bf16 stream under attn_flags 8192: each
    refused with its code, with real device buffers, and nothing written"""
    cid = next(c for c in CASES if c.startswith("dense_B2_H3") and c.endswith("p0.0"))
    c, resid, _ = _data(cid)
    geo, ins, d = _geo(c, cid), _inputs(c, False), c.H * DH
    rin = _View(_buf(c.Rq, d, NAN, pad=0), 0, c.Rq, d).put(resid)
    both = torch.full((2 * c.Rq + SLACK, d), SENT, dtype=torch.bfloat16, device=DEV)
    rout, o = _View(both, 0, c.Rq, d, 0, nbytes=c.Rq * d * 2), _View(both, 0, c.Rq, d, c.Rq)
    lse = torch.full((geo.B * geo.H * geo.Sq,), SENT, dtype=torch.float32, device=DEV)
    kw = _entry_args(geo, ins, rin, rout, o, lse, c.scale, 0.0)

    def refused(code, flags=3, **over):
        try:
            hip.set_option("attn_flags", flags)
            rc = hip.call(ENTRY, **dict(kw, **over))
        finally:
            hip.set_option("attn_flags", 3)
        msg = hip.lib().ditto_last_error().decode()
        assert rc == code and ENTRY in msg, (rc, code, msg)
    refused(hip.ERR_SIZE, resid_out_bytes=kw["resid_out_bytes"] - 1)
    refused(hip.ERR_SIZE, q_bytes=kw["q_bytes"] // 2)
    refused(hip.ERR_SIZE, lse_out_bytes=kw["lse_out_bytes"] - 4)
    refused(hip.ERR_SIZE, B=geo.B + 1)
    refused(hip.ERR_SHAPE, ldk=kw["ldk"] + 4)
    refused(hip.ERR_SHAPE, dh=128)
    refused(hip.ERR_ARG, lse_out=None)
    refused(hip.ERR_ARG, flags=8192)
    torch.cuda.synchronize()
    assert bool((both == SENT).all()) and bool((lse == SENT).all()), "a refused call wrote"
