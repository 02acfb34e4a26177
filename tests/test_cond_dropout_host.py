"""Condition dropout and the text gradient on the host (no GPU): the layout function, the argument checks of train_forward_packed's
new arguments — each decided before any launch — and the symbol table of include/ditto_text_grad.h."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from ditto_tts_amd import hip
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.varlen import cond_dropout_layout

CU_T = [0, 96, 136, 201, 202]          # text lengths 96, 40, 65, 1


@pytest.mark.parametrize("drop,T0,lens", [
    ([0, 0, 0, 0], 33, [96, 40, 65, 1]),           # none dropped: the text's own layout
    ([1, 1, 1, 1], 33, [33, 33, 33, 33]),          # all dropped
    ([1, 0, 0, 0], 33, [33, 40, 65, 1]),           # the first
    ([0, 0, 0, 1], 33, [96, 40, 65, 33]),          # the last; T0 longer than the utterance's one row
    ([0, 1, 0, 0], 130, [96, 130, 65, 1]),         # T0 longer than every text: max_T' is the null's
    ([0, 1, 0, 0], 1, [96, 1, 65, 1]),             # T0 shorter
    ([True, True, False, True], 5, [5, 5, 65, 5]),
])
def test_cond_dropout_layout(drop, T0, lens):
    for d in (drop, tuple(drop), torch.tensor(drop, dtype=torch.bool), torch.tensor(drop, dtype=torch.int64)):
        for cu_t in (CU_T, torch.tensor(CU_T, dtype=torch.int32)):
            cu_out, table, max_t = cond_dropout_layout(cu_t, d, T0)
            want = [0]
            for n in lens:
                want.append(want[-1] + n)
            assert cu_out.dtype == torch.int32 and cu_out.device.type == "cpu" and cu_out.tolist() == want
            assert max_t == max(lens) and int(cu_out[-1]) == sum(lens)
            assert table.dtype == torch.int32 and table.is_contiguous()
            assert table.tolist() == want + CU_T + [int(bool(v)) for v in drop]


@pytest.mark.parametrize("cu_t,drop,T0,why", [
    (CU_T, [0, 1, 0], 3, r"shape \[4\]"),                       # drop of the wrong length
    (CU_T, [0, 1, 0, 0, 1], 3, r"shape \[4\]"),
    (CU_T, [0, 2, 0, 0], 3, "False / True"),
    (CU_T, [0.0, 1.0, 0.0, 0.0], 3, "bools"),
    (CU_T, torch.tensor([0.0, 1.0, 0.0, 0.0]), 3, "bool or integer"),
    (CU_T, "0100", 3, "list, tuple"),
    (CU_T, [0, 1, 0, 0], 0, "at least one row"),
    (CU_T, [0, 1, 0, 0], -2, "at least one row"),
    ([0, 96, 96, 201, 202], [0, 1, 0, 0], 3, "increase"),       # an empty utterance
    ([1, 96, 136, 201, 202], [0, 1, 0, 0], 3, "start"),
])
def test_cond_dropout_layout_rejects(cu_t, drop, T0, why):
    with pytest.raises(ValueError, match=why):
        cond_dropout_layout(cu_t, drop, T0)


def _args():
    x, text, t = torch.randn(10, 256), torch.randn(6, 256), torch.tensor([1, 2])
    return x, [0, 4, 10], text, [0, 2, 6], t


def test_new_arguments_are_checked_before_the_device():
    m = DiTTO(256, 1, 4, 256, 256, 10)
    x, cu, text, cu_t, t = _args()
    null = torch.nn.Parameter(torch.randn(3, 256))
    bad = [(dict(null_text_emb=null), "together"),                                   # one of the pair without the other
           (dict(drop=[0, 1]), "together"),
           (dict(null_text_emb=null, drop=[0, 1, 0]), r"drop: shape \[2\]"),          # drop of the wrong length
           (dict(null_text_emb=null, drop=torch.tensor([True])), r"drop: shape \[2\]"),
           (dict(null_text_emb=torch.randn(3, 128), drop=[0, 1]), "null_text_emb"),   # wrong width
           (dict(null_text_emb=torch.randn(1, 3, 256), drop=[0, 1]), "null_text_emb"),  # wrong rank
           (dict(null_text_emb=torch.randn(256), drop=[0, 1]), "null_text_emb"),
           (dict(null_text_emb=torch.randn(0, 256), drop=[0, 1]), "null_text_emb")]   # T0 = 0
    for kw, why in bad:
        with pytest.raises(ValueError, match=why):
            m.train_forward_packed(x, cu, text, cu_t, t, **kw)
    # sound new arguments on CPU tensors: the device is the only thing left to refuse
    for kw in (dict(null_text_emb=null, drop=[0, 1]), dict(null_text_emb=null, drop=torch.tensor([True, False])), {}):
        with pytest.raises(RuntimeError, match="no CPU"):
            m.train_forward_packed(x, cu, text.clone().requires_grad_(True), cu_t, t, **kw)   # text_emb.requires_grad is allowed here
    with pytest.raises(NotImplementedError, match="detach"):                          # ... x's gradient stays refused, same message
        m.train_forward_packed(x.clone().requires_grad_(True), cu, text, cu_t, t, null_text_emb=null, drop=[0, 1])
    assert "null_text_emb" not in m.state_dict() and all("null" not in k for k in m.state_dict())


def test_padded_convenience_passes_the_pair_through():
    m = DiTTO(256, 1, 4, 256, 256, 10)
    x, text, t = torch.randn(2, 8, 256), torch.randn(2, 5, 256), torch.tensor([1, 2])
    null = torch.randn(3, 256)
    with pytest.raises(ValueError, match="together"):
        m.train_forward(x, text, t, speech_lengths=[8, 3], text_lengths=[5, 2], drop=[0, 1])
    with pytest.raises(RuntimeError, match="no CPU"):
        m.train_forward(x, text, t, speech_lengths=[8, 3], text_lengths=[5, 2], null_text_emb=null, drop=[0, 1])


def test_condition_dropout_mask_is_drawn_from_the_cpu_generator():
    g = torch.Generator().manual_seed(5)
    a = DiTTO.condition_dropout_mask(64, 0.5, generator=g)
    b = DiTTO.condition_dropout_mask(64, 0.5, generator=torch.Generator().manual_seed(5))
    assert a.dtype == torch.bool and a.device.type == "cpu" and a.shape == (64,) and torch.equal(a, b)
    assert 10 < int(a.sum()) < 54
    torch.manual_seed(9)
    c = DiTTO.condition_dropout_mask(16, 0.3)
    torch.manual_seed(9)
    assert torch.equal(c, DiTTO.condition_dropout_mask(16, 0.3))
    assert not DiTTO.condition_dropout_mask(8, 0.0).any() and DiTTO.condition_dropout_mask(8, 1.0).all()
    for B, p in ((0, 0.5), (4, 1.5), (4, -0.1)):
        with pytest.raises(ValueError):
            DiTTO.condition_dropout_mask(B, p)


def test_text_grad_header_declared_exported_and_bound():
    """include/ditto_text_grad.h, a table of its own beside ditto_hip.h's: declared = exported = bound; ditto_hip.h keeps its 143"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ditto_text_grad.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ditto_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["ditto_text_select_packed", "ditto_text_select_packed_bwd", "ditto_train_backward_packed_text_layers",
                     "ditto_train_workspace_bytes_packed_text"]
    assert sorted(hip.TEXT_GRAD_PROTOTYPES) == sorted(hip.TEXT_GRAD_SYMBOLS) == names
    assert not set(names) & (set(hip.SYMBOLS) | set(hip.OPTIM_SYMBOLS) | set(hip.TRAIN_ROWS_SYMBOLS))
    assert len(hip.PROTOTYPES) == 143 and len(hip.TRAIN_ROWS_PROTOTYPES) == 15
    lib = hip.lib()
    assert lib.ditto_abi_version() == 10
    for n in names:
        fn = getattr(lib, n)                                                         # AttributeError: declared but not exported
        res, params = hip.TEXT_GRAD_PROTOTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [t for _, t in params], n
        pnames = [p for p, _ in params]
        assert len(set(pnames)) == len(pnames), n
    for n in names[:2]:                                                               # the select entries: every pointer with its byte size
        params = hip.TEXT_GRAD_PROTOTYPES[n][1]
        for i, (p, t) in enumerate(params):
            if t is C.c_void_p and p != "stream":
                assert params[i + 1] == (p + "_bytes", C.c_size_t), (n, p)
    # the backward entry: ditto_train_backward_packed_layers' parameters, then the text gradient's buffer and its size
    base = hip.PROTOTYPES["ditto_train_backward_packed_layers"]
    res, params = hip.TEXT_GRAD_PROTOTYPES["ditto_train_backward_packed_text_layers"]
    assert res is base[0] and params[:-2] == base[1] and params[-2:] == [("d_text", C.c_void_p), ("d_text_bytes", C.c_size_t)]
    assert hip.TEXT_GRAD_PROTOTYPES["ditto_train_workspace_bytes_packed_text"] == \
        (C.c_size_t, hip.PROTOTYPES["ditto_train_workspace_bytes_packed"][1])


def test_text_grad_entries_refuse_on_the_host():
    """what needs no device: the workspace grows by the two buffers only; a null d_text and the select entries' shapes and tables are
    answered before any HIP call, naming the entry"""
    lib = hip.lib()
    from ditto_tts_amd.config import DiTTOConfig
    c = hip.make_config(DiTTOConfig(256, 3, 4, 256, 256, 50))
    plain = lib.ditto_train_workspace_bytes_packed(C.byref(c), 3, 407, 200, 201, 96)
    with_text = lib.ditto_train_workspace_bytes_packed_text(C.byref(c), 3, 407, 200, 201, 96)
    assert plain > 0 and with_text - plain == 256 * 512 * 2 + 3 * 256 * 4               # WkvT bf16 [dt, 2d] + dpooled fp32 [B, dt]
    assert lib.ditto_train_workspace_bytes_packed_text(C.byref(c), 3, 407, 200, 2, 96) == 0
    rc = lib.ditto_train_backward_packed_text_layers(*([None] * 7), 3, 407, 200, 201, 96, None, None, 0.0, 0, None, 0, None, None, 0,
                                                     None, None, 2, 0, None, 0)
    assert rc == hip.ERR_ARG and b"ditto_train_backward_packed_text_layers" in lib.ditto_last_error()
    _, table, _ = cond_dropout_layout([0, 2, 6], [0, 1], 3)
    kw = dict(text=None, text_bytes=0, null_rows=None, null_rows_bytes=0, table=None, table_bytes=0, table_host=table.data_ptr(),
              table_host_bytes=table.numel() * 4, text_eff=None, text_eff_bytes=0, B=2, S_T=6, S_out=5, T0=3, dt=256, stream=None)
    assert hip.call("ditto_text_select_packed", **kw) == hip.ERR_ARG and b"ditto_text_select_packed: null text" in lib.ditto_last_error()
    assert hip.call("ditto_text_select_packed", **dict(kw, dt=130)) == hip.ERR_SHAPE
    assert hip.call("ditto_text_select_packed", **dict(kw, S_out=6)) == hip.ERR_SHAPE and b"offsets" in lib.ditto_last_error()
    assert hip.call("ditto_text_select_packed", **dict(kw, T0=4)) == hip.ERR_SHAPE and b"utterance 1 (dropped)" in lib.ditto_last_error()
    assert hip.call("ditto_text_select_packed", **dict(kw, table_host_bytes=28)) == hip.ERR_SIZE
    assert hip.call("ditto_text_select_packed", **dict(kw, table_host=None)) == hip.ERR_ARG
    bad = table.clone(); bad[7] = 2                                                    # drop[1] = 2
    assert hip.call("ditto_text_select_packed", **dict(kw, table_host=bad.data_ptr())) == hip.ERR_SHAPE
    with pytest.raises(TypeError, match="ditto_text_grad.h declares no such entry"):
        hip.call("ditto_text_select_packe", **kw)
