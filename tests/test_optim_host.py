"""The fused optimizer on a GPU-less host: include/ditto_optim.h is parsed into a table of its own, exported and bound, and leaves
ditto_hip.h's 143 functions alone; the C entries' argument refusals (no launch is made: every call here fails its checks first); the
constructor's refusals; the state's key layout beside torch.optim.AdamW's; the table builder's chunk bases on hand-written sizes."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import ROOT
from ditto_tts_amd import hip, optim


def _declared():
    txt = open(os.path.join(ROOT, "include", "ditto_optim.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ditto_optim_[a-z0-9_]+)\s*\(", txt)))


def test_header_is_parsed_exported_and_bound_beside_ditto_hip_h():
    names = _declared()
    assert names == ["ditto_optim_adamw_step", "ditto_optim_grad_norm", "ditto_optim_scratch_bytes", "ditto_optim_swap"]
    assert sorted(hip.OPTIM_PROTOTYPES) == names
    lib = hip.lib()
    for n in names:
        res, params = hip.OPTIM_PROTOTYPES[n]
        pn = [q for q, _ in params]
        assert len(set(pn)) == len(pn) and all(q.isidentifier() for q in pn), n
        fn = getattr(lib, n)                                     # exported ...
        assert fn.restype == res and list(fn.argtypes) == [t for _, t in params], n      # ... and bound
        assert n not in hip.SYMBOLS and n not in hip.PROTOTYPES
    assert len(hip.PROTOTYPES) == 143 and len(hip.SYMBOLS) == 143
    assert lib.ditto_abi_version() == 10
    assert hip.OPTIM_PROTOTYPES["ditto_optim_scratch_bytes"] == (C.c_size_t, [("n_chunks", C.c_size_t)])
    assert [q for q, _ in hip.OPTIM_PROTOTYPES["ditto_optim_adamw_step"][1]] == [
        "table", "n_seg", "n_chunks", "hyper", "state", "phase", "scratch", "scratch_bytes", "grid_limit", "stream"]


def test_struct_layouts_match_the_header():
    assert C.sizeof(hip.OptimSeg) == 72 == optim.SEG_DTYPE.itemsize
    assert [(n, optim.SEG_DTYPE.fields[n][1]) for n in optim.SEG_DTYPE.names] == \
        [(n, getattr(hip.OptimSeg, n).offset) for n, _ in hip.OptimSeg._fields_]
    assert C.sizeof(hip.OptimHyper) == 48
    blk = optim.state_block(0.9, 0.999, 3, 2)
    assert len(blk) == hip.OPTIM_STATE_BYTES == 128
    p1, p2, step, skipped = struct.unpack_from("<ddqq", blk, 0)
    assert (p1, p2, step, skipped) == (0.9 * 0.9 * 0.9, 0.999 * 0.999 * 0.999, 3, 2) and blk[:32] == blk[32:64]
    assert struct.unpack_from("<f", blk, hip.OPTIM_STATE_CLIP) == (1.0,) and struct.unpack_from("<i", blk, hip.OPTIM_STATE_SKIP) == (0,)
    txt = open(os.path.join(ROOT, "ditto_tts_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"#define DITTO_OPTIM_CHUNK_QUADS (\d+)", txt).group(1)) == hip.OPTIM_CHUNK_QUADS


def _step(**over):
    kw = dict(table=256, n_seg=2, n_chunks=2, hyper=hip.OptimHyper(0.9, 0.999, 1e-8, 1.0, 0.99, 1, 0), state=256, phase=0,
              scratch=256, scratch_bytes=256, grid_limit=0, stream=None)
    kw.update(over)
    return hip.call("ditto_optim_adamw_step", **kw)


@pytest.mark.parametrize("over,code,word", [
    (dict(table=None), hip.ERR_ARG, "null table"), (dict(hyper=None), hip.ERR_ARG, "null hyper"),
    (dict(state=None), hip.ERR_ARG, "null state"), (dict(scratch=None), hip.ERR_ARG, "null scratch"),
    (dict(n_seg=0), hip.ERR_ARG, "n_seg"), (dict(n_seg=65536, n_chunks=65536), hip.ERR_ARG, "n_seg"),
    (dict(n_chunks=1), hip.ERR_ARG, "n_chunks"), (dict(n_chunks=2 ** 31), hip.ERR_ARG, "n_chunks"),
    (dict(phase=-1), hip.ERR_ARG, "phase"), (dict(grid_limit=-1), hip.ERR_ARG, "grid_limit"),
    (dict(state=264), hip.ERR_ARG, "16-byte"), (dict(scratch=272), hip.ERR_ARG, "256-byte"),
    (dict(n_chunks=40, scratch_bytes=256), hip.ERR_SIZE, "scratch too small"),
    (dict(hyper=hip.OptimHyper(1.0, 0.999, 1e-8, 1.0, 0.99, 1, 0)), hip.ERR_ARG, "betas"),
    (dict(hyper=hip.OptimHyper(0.9, float("nan"), 1e-8, 1.0, 0.99, 1, 0)), hip.ERR_ARG, "betas"),
    (dict(hyper=hip.OptimHyper(0.9, 0.999, -1.0, 1.0, 0.99, 1, 0)), hip.ERR_ARG, "eps"),
    (dict(hyper=hip.OptimHyper(0.9, 0.999, float("inf"), 1.0, 0.99, 1, 0)), hip.ERR_ARG, "eps"),
    (dict(hyper=hip.OptimHyper(0.9, 0.999, 1e-8, float("inf"), 0.99, 1, 0)), hip.ERR_ARG, "max_norm"),
    (dict(hyper=hip.OptimHyper(0.9, 0.999, 1e-8, 1.0, 1.5, 1, 0)), hip.ERR_ARG, "ema_decay"),
    (dict(hyper=hip.OptimHyper(0.9, 0.999, 1e-8, 1.0, 0.99, 2, 0)), hip.ERR_ARG, "skip_nonfinite"),
])
def test_step_entry_refuses_before_any_launch(over, code, word):
    assert _step(**over) == code
    assert word in hip.lib().ditto_last_error().decode()


def test_other_entries_refuse_and_call_is_by_name():
    h = hip.OptimHyper(0.9, 0.999, 1e-8, 1.0, 0.99, 1, 0)
    assert hip.call("ditto_optim_grad_norm", table=None, n_seg=1, n_chunks=1, hyper=h, state=256, scratch=256, scratch_bytes=256,
                    grid_limit=0, stream=None) == hip.ERR_ARG
    assert hip.call("ditto_optim_grad_norm", table=256, n_seg=1, n_chunks=1, hyper=h, state=256, scratch=256, scratch_bytes=8,
                    grid_limit=0, stream=None) == hip.ERR_SIZE
    assert hip.call("ditto_optim_swap", table=None, n_seg=1, n_chunks=1, grid_limit=0, stream=None) == hip.ERR_ARG
    assert hip.call("ditto_optim_swap", table=256, n_seg=3, n_chunks=2, grid_limit=0, stream=None) == hip.ERR_ARG
    lib = hip.lib()
    assert lib.ditto_optim_scratch_bytes(0) == 0 and b"n_chunks" in lib.ditto_last_error()
    assert lib.ditto_optim_scratch_bytes(1) == 256 and lib.ditto_optim_scratch_bytes(33) == 512
    with pytest.raises(TypeError, match="ditto_optim_swap: missing stream"):
        hip.call("ditto_optim_swap", table=256, n_seg=1, n_chunks=1, grid_limit=0)
    with pytest.raises(TypeError, match="ditto_optim_nothing: include/ditto_optim.h declares no such entry"):
        hip.call("ditto_optim_nothing")


def test_chunk_bases_on_hand_written_sizes():
    E = 4 * hip.OPTIM_CHUNK_QUADS                                 # elements of a chunk
    assert [hip.optim_chunks(n) for n in (1, 3, 4, 5, E - 1, E, E + 1, 2 * E, 2 * E + 1, 3 * E + 5)] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 4]
    assert optim.chunk_bases([1, E, E + 1, 5, 3 * E + 5]) == ([0, 1, 2, 4, 5], 9)
    with pytest.raises(ValueError):
        optim.chunk_bases([4, 0])
    rows = np.zeros(3, dtype=optim.SEG_DTYPE)
    total = optim.fill_table(rows, ([16, 32, 48], [1, 2, 3], [4, 5, 6], [7, 8, 9], [0, 10, 0]), [E + 1, 7, E], [1e-3, 2e-3, 1e-3],
                             [0.0, 0.1, 0.0])
    assert total == 4 and rows["slot0"].tolist() == [0, 2, 3] and rows["n"].tolist() == [E + 1, 7, E]
    assert rows["ema"].tolist() == [0, 10, 0] and rows["lr"].tolist() == [1e-3, 2e-3, 1e-3]
    seg = hip.OptimSeg.from_buffer_copy(rows.tobytes()[72:144])
    assert (seg.p, seg.g, seg.m, seg.v, seg.ema, seg.n, seg.slot0, seg.lr, seg.weight_decay) == (32, 2, 5, 8, 10, 7, 2, 2e-3, 0.1)


def test_constructor_refusals_name_what_is_wrong():
    w = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="CPU path"):
        optim.AdamW([w])
    with pytest.raises(ValueError, match=r"parameter 'blocks.0.w'.*CPU path"):
        optim.AdamW([("blocks.0.w", w)])
    with pytest.raises(ValueError, match="fp32 parameters only"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([w], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.AdamW([w], maximize=True)
    with pytest.raises(ValueError, match="betas"):
        optim.AdamW([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(4))], "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="eps"):
        optim.AdamW([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(4))], "eps": 1e-6}])
    for kw, word in ((dict(betas=(0.9, 1.0)), "betas"), (dict(eps=-1.0), "eps"), (dict(max_norm=0.0), "max_norm"),
                     (dict(max_norm=float("inf")), "max_norm"), (dict(ema_decay=1.5), "ema_decay"), (dict(lr=-1.0), "lr")):
        with pytest.raises(ValueError, match=word):
            optim.AdamW([w], **kw)


def test_state_keys_are_torchs_plus_the_average():
    w = torch.nn.Parameter(torch.ones(6))
    t = torch.optim.AdamW([w], foreach=False)
    w.grad = torch.ones(6)
    t.step()
    sd = t.state_dict()
    assert tuple(sd["state"][0]) == optim.STATE_KEYS                       # step, exp_avg, exp_avg_sq: the layout ours is read from
    st = optim.new_state(w, ema=True)
    assert tuple(st) == optim.STATE_KEYS + (optim.EMA_KEY,) and tuple(optim.new_state(w, ema=False)) == optim.STATE_KEYS
    assert st["step"].shape == sd["state"][0]["step"].shape and st["step"].dtype == sd["state"][0]["step"].dtype
    assert torch.equal(st["ema"], w.detach()) and st["ema"].data_ptr() != w.data_ptr()
    assert float(st["exp_avg"].abs().sum()) == 0.0 and st["exp_avg_sq"].shape == w.shape
