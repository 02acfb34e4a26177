"""Guidance rescale on the host (no GPU): the validation of sample_guided_packed(guidance_rescale=) and
GuidedStream.submit(guidance_rescale=), the padded entries' NotImplementedError, the new symbols (exported, bound, ABI still 10),
ditto_guidance_rescale_bytes' arithmetic and the entries' argument checks, phi in the stream's step arguments, and the step block:
its existing fields keep the offsets they had before phi was appended."""
import ctypes as C

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import rescale_vector
from ditto_tts_amd.serving import step_block_layout
from test_cabi_symbols import declared_functions
from test_interval_host import _bare_generator
from test_stream_host import TEXT_DIM, _stream

NEW = ("ditto_guidance_rescale_bytes", "ditto_guidance_rescale_packed", "ditto_guided_step_packed_rescale_opts",
       "ditto_guided_step_packed_multistep_rescale_opts")
P = 4096   # a non-NULL, 256-byte aligned pointer value: every call below fails its argument checks before anything touches it


def test_rescale_vector():
    assert rescale_vector(None, 3) is None
    assert rescale_vector(0.7, 3).tolist() == pytest.approx([0.7] * 3) and rescale_vector(1, 2).tolist() == [1.0, 1.0]
    assert rescale_vector([0.7, 0.0, 0.3], 3).dtype == torch.float32
    assert rescale_vector(torch.tensor([0.0, 1.0]), 2).tolist() == [0.0, 1.0]
    for bad in (-0.1, 1.5, float("nan"), float("inf"), True, "a", [0.5, 2.0, 0.1], [0.5, None, 0.1], (0.1, True, 0.2)):
        with pytest.raises(ValueError, match="guidance_rescale"):
            rescale_vector(bad, 3)
    for bad in ([0.5, 0.5], [0.1] * 4, torch.zeros(2)):
        with pytest.raises(ValueError, match="3 values expected"):
            rescale_vector(bad, 3)


def test_closed_call_refusals_before_any_launch():
    sg = _bare_generator(DiTTOConfig(256, 2, 4, 256, 256, 50))
    audio, text = torch.zeros(15, 256), torch.zeros(9, 256)
    packed = (text, [0, 3, 6, 9], audio, [0, 5, 6, 15])
    ok = dict(guidance=2.0, null_text_emb=text)
    for solver in ("ddim", "dpmpp2m"):
        for bad in (1.5, -0.25, [0.5, 0.5], [0.1, 0.2, 3.0]):
            with pytest.raises(ValueError, match="guidance_rescale"):
                sg.sample_guided_packed(*packed, solver=solver, guidance_rescale=bad, **ok)
        with pytest.raises(ValueError, match="guidance_rescale needs guidance"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_rescale=0.7)
        with pytest.raises(ValueError, match="guidance_rescale needs guidance"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_rescale=0.7, guidance=2.0)
    # the padded layouts point to the packed call, as they do for prompts and solvers
    padded = (torch.zeros(1, 3, 256), torch.zeros(1, 5, 256))
    for entry in (sg.sample_guided, sg.sample_latents_strided):
        with pytest.raises(NotImplementedError, match="sample_guided_packed"):
            entry(*padded, guidance_rescale=0.7)
    # the existing refusals stay in front: head_dim != 64 and fp8 linears
    for cfg, word in ((DiTTOConfig(256, 2, 2, 256, 256, 50), "head_dim 64"), (DiTTOConfig(256, 2, 4, 256, 256, 50, fp8_linear=True), "fp8")):
        with pytest.raises(NotImplementedError, match=word):
            _bare_generator(cfg).sample_guided_packed(*packed, guidance_rescale=0.7, **ok)


def test_stream_submit_validation_and_step_arguments():
    s = _stream()
    text, null = torch.zeros(4, TEXT_DIM), torch.zeros(5, TEXT_DIM)
    for bad in (1.5, -0.1, True, "x", [0.5], float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.submit(text, 8, seed=1, guidance=2.0, null_text_emb=null, n_steps=3, guidance_rescale=bad)
    assert s.pending == 0                                        # a refused request leaves the stream as it was
    with pytest.raises(ValueError, match="unguided"):
        _stream(guided=False).submit(text, 8, seed=1, n_steps=3, guidance_rescale=0.5)
    s.submit(text, 8, seed=1, guidance=2.0, null_text_emb=null, n_steps=2, guidance_rescale=0.7)
    s.submit(text, 9, seed=2, guidance=3.0, null_text_emb=null, n_steps=2)
    s.submit(text, 7, seed=3, guidance=3.0, null_text_emb=null, n_steps=2, guidance_rescale=0)
    s.step()
    assert s.batch.steps[-1].phi == [0.7, 0.0, 0.0]              # in slot order, beside w


def test_symbols_exported_bound_and_abi_ten():
    lib, names = hip.lib(), declared_functions()
    for n in NEW:
        assert n in names and n in hip.SYMBOLS and hasattr(lib, n), n
    assert lib.ditto_abi_version() == 10
    assert hip.RESCALE_CHUNK_QUADS == 4096


def test_rescale_bytes_arithmetic():
    lib = hip.lib()
    al = lambda n: (n + 255) // 256 * 256
    for B, max_N, d in ((1, 1, 64), (3, 96, 256), (32, 2000, 768), (7, 64, 256), (7, 65, 256), (300, 17, 1024)):
        chunks = -(-(max_N * d // 4) // hip.RESCALE_CHUNK_QUADS)
        want = al(32 * B) + al(4 * B) + al(B * chunks * 32)       # coef_out (as ditto_multistep_coef [B]) | scale | 4 doubles a chunk
        assert lib.ditto_guidance_rescale_bytes(B, max_N, d) == want, (B, max_N, d)
        assert hip.rescale_scratch_layout(B) == (al(32 * B), al(32 * B) + al(4 * B))
    assert C.sizeof(hip.MultistepCoef) == 32
    for bad in ((0, 5, 64), (2, 0, 64), (2, 5, 0), (2, 5, 96)):
        assert lib.ditto_guidance_rescale_bytes(*bad) == 0
        assert b"ditto_guidance_rescale_bytes" in lib.ditto_last_error()


def test_entry_argument_checks_before_any_launch():
    lib = hip.lib()
    need = lib.ditto_guidance_rescale_bytes(3, 9, 256)

    def call(**kw):
        a = dict(eps2=P, w=P, phi=P, coef_in=P, coefs=None, cu=P, prompt_len=None, partner=None, B=3, G=0, S=15, S_G=0, max_N=9, d=256,
                 scratch=P, scratch_bytes=need)
        a.update(kw)
        return lib.ditto_guidance_rescale_packed(a["eps2"], a["w"], a["phi"], a["coef_in"], a["coefs"], a["cu"], a["prompt_len"],
                                                 a["partner"], a["B"], a["G"], a["S"], a["S_G"], a["max_N"], a["d"], a["scratch"],
                                                 a["scratch_bytes"], None)

    for kw, code, word in ((dict(eps2=None), hip.ERR_ARG, b"null"), (dict(phi=None), hip.ERR_ARG, b"null"),
                           (dict(scratch=None), hip.ERR_ARG, b"null"), (dict(coef_in=None), hip.ERR_ARG, b"exactly one"),
                           (dict(coefs=P), hip.ERR_ARG, b"exactly one"), (dict(w=None), hip.ERR_ARG, b"needs w"),
                           (dict(coef_in=None, coefs=P + 8), hip.ERR_ARG, b"16-byte"), (dict(scratch=P + 16), hip.ERR_ARG, b"256-byte"),
                           (dict(d=96), hip.ERR_SHAPE, b"% 64"), (dict(max_N=16), hip.ERR_SHAPE, b"max_N <= S"),
                           (dict(partner=P, G=4, S_G=4), hip.ERR_SHAPE, b"G <= B"), (dict(partner=P, G=0, S_G=4), hip.ERR_SHAPE, b"S_G"),
                           (dict(scratch_bytes=need - 1), hip.ERR_SIZE, b"ditto_guidance_rescale_bytes")):
        assert call(**kw) == code, kw
        assert word in lib.ditto_last_error(), (kw, lib.ditto_last_error())
    # the step entries refuse a null model before anything else
    assert lib.ditto_guided_step_packed_rescale_opts(None, *([P] * 9), 0, *([P] * 6), 3, 0, 15, 0, 9, 9, 3, P, P, P, 1 << 20, P, need, None,
                                                     None) == hip.ERR_ARG
    assert lib.ditto_guided_step_packed_multistep_rescale_opts(None, *([P] * 9), 3, 15, 9, 9, 3, P, P, P, 1 << 20, P, need, None,
                                                               None) == hip.ERR_ARG


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("multistep", [True, False])
@pytest.mark.parametrize("maxB", [1, 3, 4, 13, 32])
def test_step_block_fields_keep_their_offsets(maxB, guided, multistep):
    """the layout as it stood before phi was appended, restated"""
    pad = lambda n, m: (n + m - 1) // m * m
    lay = step_block_layout(maxB, guided, multistep)
    nbB = (2 if guided else 1) * maxB
    o_seeds = pad(nbB * 8, 16)
    o_f, stride = o_seeds + pad(maxB * 8, 16), pad(maxB * 4, 16)
    old = dict(t=0, seeds=o_seeds, f_stride=stride)
    for k, name in enumerate(("a", "ce", "cz", "w", "tags", "prompt", "partner", "coef")):
        old[name] = o_f + k * stride
    for name, at in old.items():
        assert lay[name] == at, name
    old_bytes = old["coef"] + (32 * maxB if multistep else 0)
    assert lay["phi"] >= old_bytes and lay["phi"] % 16 == 0 and lay["bytes"] == lay["phi"] + stride
