"""Variable-length batches on the host (no GPU): the C entry points are declared, exported and bound; they refuse bad arguments with
an error code and a message before any launch; the length validation of ditto_tts_amd.varlen rejects what the kernels must not see."""
import pytest
import torch

from ditto_tts_amd import hip, varlen
from test_cabi_symbols import declared_functions

VARLEN_ENTRIES = ("ditto_attention_varlen_bf16", "ditto_attention_resid_varlen_bf16")
P = 4096   # a non-NULL pointer value: every call below fails its argument checks before anything touches it


def test_varlen_symbols_declared_exported_and_bound():
    lib = hip.lib()
    names = declared_functions()
    for n in VARLEN_ENTRIES:
        assert n in names and hasattr(lib, n) and n in hip.SYMBOLS
    assert hip.has_varlen()
    assert lib.ditto_abi_version() == 10


def _plain(lib, q=P, out=P, ql=P, kl=P, B=2, Hh=2, Sq=128, Skv=128, dh=64, ld=128):
    return lib.ditto_attention_varlen_bf16(q, ld, P, ld, P, ld, out, ld, ql, kl, B, Hh, Sq, Skv, dh, None)


def _resid(lib, q=P, out=P, ql=P, kl=P, B=2, Hh=2, Sq=128, Skv=128, dh=64, ld=128):
    return lib.ditto_attention_resid_varlen_bf16(q, ld, P, ld, P, ld, None, out, ld, 0, ql, kl, B, Hh, Sq, Skv, dh, None)


@pytest.mark.parametrize("call", [_plain, _resid], ids=["plain", "resid"])
def test_varlen_entries_refuse_bad_arguments(call):
    lib = hip.lib()
    for kw, code, word in [(dict(q=None), hip.ERR_ARG, b"null"), (dict(out=None), hip.ERR_ARG, b"null"),
                           (dict(ql=None, kl=None), hip.ERR_ARG, b"NULL"), (dict(B=0), hip.ERR_SHAPE, b"positive"),
                           (dict(B=-3), hip.ERR_SHAPE, b"positive"), (dict(Sq=0), hip.ERR_SHAPE, b"positive"),
                           (dict(dh=128, ld=256), hip.ERR_SHAPE, b"head_dim 64"), (dict(dh=72, ld=144), hip.ERR_SHAPE, b"head_dim 64"),
                           (dict(ld=100), hip.ERR_SHAPE, b"multiples of 8")]:
        assert call(lib, **kw) == code, kw
        assert word in lib.ditto_last_error(), (kw, lib.ditto_last_error())


def test_validate_lengths_accepts_lists_tuples_and_int_tensors():
    for v in ([1, 5, 7], (1, 5, 7), torch.tensor([1, 5, 7]), torch.tensor([1, 5, 7], dtype=torch.int32),
              torch.tensor([1, 5, 7], dtype=torch.int16)):
        t = varlen.validate_lengths(v, 3, 7)
        assert t.dtype == torch.int32 and t.device.type == "cpu" and t.tolist() == [1, 5, 7]


@pytest.mark.parametrize("bad", [[1, 2], [[1, 2, 3]], torch.ones(3, 1, dtype=torch.int64), torch.tensor([1.0, 2.0, 3.0]),
                                 [1, 2.0, 3], [0, 2, 3], [1, 2, 8], [-1, 2, 3], torch.tensor([1, 8, 2]), "123", None,
                                 [True, True, True]],
                         ids=["short", "nested", "2d", "float_tensor", "float_item", "zero", "above_N", "negative",
                              "tensor_above_N", "string", "none", "bool"])
def test_validate_lengths_rejects(bad):
    with pytest.raises(ValueError):
        varlen.validate_lengths(bad, 3, 7)


def test_model_level_varlen_entries_refuse_null_lengths():
    lib = hip.lib()
    for n in ("ditto_text_precompute_varlen", "ditto_forward_varlen_opts", "ditto_p_sample_varlen_opts",
              "ditto_p_sample_seeded_varlen_opts"):
        assert n in declared_functions() and n in hip.SYMBOLS and hasattr(lib, n)
    assert lib.ditto_text_precompute_varlen(P, P, None, 2, 64, P, 1 << 30, P, 1 << 30, None) == hip.ERR_ARG
    assert b"text_len" in lib.ditto_last_error()
    assert lib.ditto_forward_varlen_opts(P, P, P, P, None, P, 2, 64, 64, P, P, P, P, 1 << 30, None, None) == hip.ERR_ARG
    assert lib.ditto_forward_varlen_opts(P, P, P, P, P, None, 2, 64, 64, P, P, P, P, 1 << 30, None, None) == hip.ERR_ARG
    assert lib.ditto_p_sample_varlen_opts(P, P, P, P, P, None, P, P, P, P, 2, 64, 64, P, P, P, 1 << 30, None, None) == hip.ERR_ARG
    assert lib.ditto_p_sample_seeded_varlen_opts(P, P, P, P, P, P, None, 0, P, P, P, 2, 64, 64, P, P, P, 1 << 30, None,
                                                 None) == hip.ERR_ARG
    assert lib.ditto_p_sample_seeded_varlen_opts(P, P, P, P, P, P, P, 0, P, P, P, 0, 64, 64, P, P, P, 1 << 30, None,
                                                 None) == hip.ERR_SHAPE
