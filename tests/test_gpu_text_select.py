"""-m gpu: condition dropout's two kernels, one launch each (ditto_text_select_packed / ditto_text_select_packed_bwd,
include/ditto_text_grad.h, csrc/text_grad.hip), bit for bit against slices assembled on the CPU.

Every output lies inside a larger allocation with GUARD elements of a bit pattern before and after it: the pattern must survive.  The
forward and d_text are copies, so torch.equal; d_null is a sum of fp32 rows in ascending utterance order from one accumulator per
element, which a sequential fp32 loop on the CPU reproduces exactly — no tolerance anywhere in this file.  Refused calls are made on
pattern-filled outputs, which must still carry the pattern afterwards: nothing was launched."""
import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.synth import hash_normal
from ditto_tts_amd.varlen import cond_dropout_layout
from gpu_util import stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
PAT = 0x7FC0BEEF          # a NaN with a payload: an output that still holds it was not written
TL = [96, 40, 65, 1]
DROPS = {"none": [0, 0, 0, 0], "one": [0, 1, 0, 0], "three": [1, 1, 0, 1], "all": [1, 1, 1, 1]}


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


class Out:
    """an fp32 output [rows, dt] inside pattern guards"""

    def __init__(self, rows, dt):
        self.n = rows * dt
        self.buf = torch.full((self.n + 2 * GUARD,), PAT, dtype=torch.int32, device=DEV)
        self.v = self.buf[GUARD:GUARD + self.n].view(torch.float32).view(rows, dt)

    def guards_clean(self):
        return bool((self.buf[:GUARD] == PAT).all()) and bool((self.buf[GUARD + self.n:] == PAT).all())

    def untouched(self):
        return bool((self.buf == PAT).all())


def _select(text_t, null_t, table_t, out, **over):
    """the forward entry on these tensors (`over`: arguments replaced, by the header's names); returns its status"""
    tdev = table_t.to(DEV)
    kw = dict(text=text_t.data_ptr(), text_bytes=text_t.numel() * 4, null_rows=null_t.data_ptr(), null_rows_bytes=null_t.numel() * 4,
              table=tdev.data_ptr(), table_bytes=tdev.numel() * 4, table_host=table_t.data_ptr(), table_host_bytes=table_t.numel() * 4,
              text_eff=out.v.data_ptr(), text_eff_bytes=out.n * 4, B=(table_t.numel() - 2) // 3, S_T=text_t.shape[0],
              S_out=out.v.shape[0], T0=null_t.shape[0], dt=text_t.shape[1], stream=stream())
    kw.update(over)
    rc = hip.call("ditto_text_select_packed", **kw)
    torch.cuda.synchronize()
    return rc


def _select_bwd(g_t, table_t, d_text_o, d_null_o, **over):
    tdev = table_t.to(DEV)
    kw = dict(d_text_eff=g_t.data_ptr(), d_text_eff_bytes=g_t.numel() * 4, table=tdev.data_ptr(), table_bytes=tdev.numel() * 4,
              table_host=table_t.data_ptr(), table_host_bytes=table_t.numel() * 4, d_text=d_text_o.v.data_ptr(),
              d_text_bytes=d_text_o.n * 4, d_null=d_null_o.v.data_ptr(), d_null_bytes=d_null_o.n * 4, B=(table_t.numel() - 2) // 3,
              S_T=d_text_o.v.shape[0], S_out=g_t.shape[0], T0=d_null_o.v.shape[0], dt=g_t.shape[1], stream=stream())
    kw.update(over)
    rc = hip.call("ditto_text_select_packed_bwd", **kw)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("drop", list(DROPS))
@pytest.mark.parametrize("T0", [1, 33, 130])
@pytest.mark.parametrize("dt", [256, 768])
def test_select_forward_and_backward_are_bit_exact(dt, T0, drop):
    d = DROPS[drop]
    cu_t = _cu(TL)
    cu_out, table, max_t = cond_dropout_layout(cu_t, d, T0)
    S_T, S_out, B = cu_t[-1], int(cu_out[-1]), len(TL)
    text = hash_normal((S_T, dt), "sel_text", dt + T0)
    null = hash_normal((T0, dt), "sel_null", dt + T0 + 1)
    # ---- forward
    want = torch.cat([null if d[b] else text[cu_t[b]:cu_t[b + 1]] for b in range(B)])
    assert want.shape == (S_out, dt)
    out = Out(S_out, dt)
    text_d, null_d = text.to(DEV), null.to(DEV)
    assert _select(text_d, null_d, table, out) == hip.OK
    assert torch.equal(out.v.cpu(), want) and out.guards_clean()
    assert torch.equal(text_d.cpu(), text) and torch.equal(null_d.cpu(), null)
    # ---- backward
    g = hash_normal((S_out, dt), "sel_g", dt + T0 + 2)
    want_text = torch.zeros(S_T, dt)
    want_null = torch.zeros(T0, dt)
    co = cu_out.tolist()
    for b in range(B):                                   # ascending b: the kernel's order
        rows = g[co[b]:co[b + 1]]
        if d[b]:
            want_null = want_null + rows                 # one fp32 add per element and utterance
        else:
            want_text[cu_t[b]:cu_t[b + 1]] = rows
    d_text, d_null = Out(S_T, dt), Out(T0, dt)
    g_d = g.to(DEV)
    assert _select_bwd(g_d, table, d_text, d_null) == hip.OK
    assert torch.equal(d_text.v.cpu(), want_text) and d_text.guards_clean()
    assert torch.equal(d_null.v.cpu(), want_null) and d_null.guards_clean()
    for b in range(B):
        if d[b]:
            assert not d_text.v[cu_t[b]:cu_t[b + 1]].any()                 # exact zeros on the dropped utterances' rows
    assert torch.equal(g_d.cpu(), g)


def test_refused_calls_launch_nothing():
    dt, T0, d = 256, 33, DROPS["one"]
    cu_t = _cu(TL)
    cu_out, table, _ = cond_dropout_layout(cu_t, d, T0)
    S_T, S_out, B = cu_t[-1], int(cu_out[-1]), len(TL)
    text, null, g = (hash_normal(s, "sel_r", 3).to(DEV) for s in ((S_T, dt), (T0, dt), (S_out, dt)))
    out, d_text, d_null = Out(S_out, dt), Out(S_T, dt), Out(T0, dt)
    lib = hip.lib()

    def bad_table(i, v):
        t = table.clone()
        t[i] = v
        return dict(table_host=t.data_ptr(), table_host_bytes=t.numel() * 4, _keep=t)

    fwd = [(dict(text_bytes=S_T * dt * 4 - 4), hip.ERR_SIZE), (dict(null_rows_bytes=T0 * dt * 4 - 4), hip.ERR_SIZE),
           (dict(text_eff_bytes=S_out * dt * 4 - 4), hip.ERR_SIZE), (dict(table_bytes=(3 * B + 2) * 4 - 4), hip.ERR_SIZE),
           (dict(table_host_bytes=(3 * B + 2) * 4 - 4), hip.ERR_SIZE), (dict(text=None), hip.ERR_ARG), (dict(table=None), hip.ERR_ARG),
           (dict(text=text.data_ptr() + 4), hip.ERR_ARG), (dict(dt=258), hip.ERR_SHAPE), (dict(T0=0), hip.ERR_SHAPE),
           (dict(T0=T0 + 1), hip.ERR_SHAPE),                   # the dropped utterance's length in the table is not T0
           (dict(S_out=S_out + 1), hip.ERR_SHAPE),             # cu_out does not end at S_out
           (bad_table(2 * B + 2, 1), hip.ERR_SHAPE),           # utterance 0 marked dropped, its length is its own
           (bad_table(2 * B + 3, 3), hip.ERR_SHAPE),           # drop = 3
           (bad_table(1, 0), hip.ERR_SHAPE),                   # cu_out does not increase
           (bad_table(B + 2, 500), hip.ERR_SHAPE)]             # cu_text out of order
    for over, code in fwd:
        keep = over.pop("_keep", None)                      # (the altered host table stays alive over the call)
        assert _select(text, null, table, out, **over) == code, over
        assert b"ditto_text_select_packed:" in lib.ditto_last_error()
        assert out.untouched(), over
    bwd = [(dict(d_text_eff_bytes=S_out * dt * 4 - 4), hip.ERR_SIZE), (dict(d_text_bytes=S_T * dt * 4 - 4), hip.ERR_SIZE),
           (dict(d_null_bytes=T0 * dt * 4 - 4), hip.ERR_SIZE), (dict(d_null=None), hip.ERR_ARG), (dict(B=0), hip.ERR_SHAPE),
           (dict(T0=T0 - 1), hip.ERR_SHAPE), (bad_table(2 * B + 3, 0), hip.ERR_SHAPE)]
    for over, code in bwd:
        keep = over.pop("_keep", None)
        assert _select_bwd(g, table, d_text, d_null, **over) == code, over
        assert b"ditto_text_select_packed_bwd:" in lib.ditto_last_error()
        assert d_text.untouched() and d_null.untouched(), over
    # and the sound calls on the same buffers still run
    assert _select(text, null, table, out) == hip.OK and not out.untouched() and out.guards_clean()
    assert _select_bwd(g, table, d_text, d_null) == hip.OK and d_text.guards_clean() and d_null.guards_clean()
