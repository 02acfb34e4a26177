"""Speech infilling on the host (no GPU): varlen.validate_suffix_lengths, a Python restatement of the device clamp of the window
(csrc/guided_update.h window_span) with the rows it documents for good and bad (P, Q), the segments of a suffixed request of a
stream (newcomer, survivor, history, retirement) and its step block, the argument refusals of the sampling surfaces and of the
stream, and the new symbols with their NULL-argument refusals."""
import ctypes as C
import types

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.serving import (_DST_OUT, _DST_Q, _DST_X, _SRC_Q, _SRC_X, _SRC_XT, GuidedStream, history_segment, retire_segments,
                                   speech_segments, staged_rows, step_block_layout)
from ditto_tts_amd.varlen import validate_prompt_lengths, validate_suffix_lengths
from test_cabi_symbols import declared_functions
from test_stream_host import TEXT_DIM, D, StubBatch, _acp

NEW = ("ditto_guided_update_packed_window", "ditto_guided_update_packed_tags_window", "ditto_guided_step_packed_window_opts",
       "ditto_guided_step_packed_tags_window_opts", "ditto_multistep_update_window", "ditto_guided_step_packed_multistep_window_opts",
       "ditto_span_noise_window", "ditto_span_mse_window")
PTR = 4096   # a non-NULL pointer value: every call below fails its argument checks before anything touches it
# bad (P, Q) pairs, shared with the GPU clamp test: negative, too large, and P + Q >= n
BAD_WINDOWS = ((-3, 2), (2, -5), (100, 0), (0, 100), (3, 100), (100, 100), (-1, -1), (2, 3))


def window_clamp(n, p, q):
    """window_span's clamp of one utterance of n >= 1 rows: P into [0, n - 1], then Q into [0, n - 1 - P]"""
    p = min(max(p, 0), n - 1)
    q = min(max(q, 0), n - 1 - p)
    return p, q


def window_of(cu, S, b, p, q):
    """(first row, one past the last row) of utterance b's window after the utterance's own clamp (utt_rows) and window_clamp"""
    r0 = min(max(cu[b], 0), S - 1)
    n = min(max(cu[b + 1] - r0, 1), S - r0)
    p, q = window_clamp(n, p, q)
    return r0 + p, r0 + n - q


def test_validate_suffix_lengths():
    cu = torch.tensor([0, 5, 6, 15], dtype=torch.int32)
    for ok in ([0, 0, 0], (4, 0, 8), torch.tensor([1, 0, 3]), torch.tensor([1, 0, 3], dtype=torch.int32)):
        out = validate_suffix_lengths(ok, cu, None)
        assert out.dtype == torch.int32 and out.device.type == "cpu" and out.tolist() == [int(v) for v in ok]
    assert validate_suffix_lengths([2, 0, 4], cu, [2, 0, 4]).tolist() == [2, 0, 4]          # P + Q = n - 1: one generated row
    assert validate_suffix_lengths([2, 0, 4], cu, torch.tensor([2, 0, 4])).tolist() == [2, 0, 4]
    for bad, pl, b in (([5, 0, 0], None, 0), ([0, 1, 0], None, 1), ([0, 0, -1], None, 2), ([3, 0, 0], [2, 0, 0], 0),
                       ([0, 0, 5], [0, 0, 4], 2)):
        with pytest.raises(ValueError, match=f"utterance {b}"):
            validate_suffix_lengths(bad, cu, pl)
    for bad in ([0, 0], [0.0, 0.0, 0.0], [True, False, True], torch.zeros(3), torch.zeros(3, dtype=torch.bool), "000", None, 3):
        with pytest.raises(ValueError):
            validate_suffix_lengths(bad, cu, None)
    with pytest.raises(ValueError, match="prompt_lengths"):                                  # the prompt lengths are validated too
        validate_suffix_lengths([0, 0, 0], cu, [5, 0, 0])
    assert validate_prompt_lengths([4, 0, 8], cu).tolist() == [4, 0, 8]                      # (unchanged)


def test_window_clamp_gives_the_documented_rows():
    # good values pass through; G >= 1 always
    for n, p, q in ((5, 0, 0), (1, 0, 0), (9, 8, 0), (7, 3, 3), (6, 0, 4), (12, 2, 3)):
        assert window_clamp(n, p, q) == (p, q)
    want = {(-3, 2): (0, 2), (2, -5): (2, 0), (100, 0): (6, 0), (0, 100): (0, 6), (3, 100): (3, 3), (100, 100): (6, 0), (-1, -1): (0, 0),
            (2, 3): (2, 3)}
    assert set(want) == set(BAD_WINDOWS)
    for (p, q), out in want.items():
        assert window_clamp(7, p, q) == out
    assert window_clamp(4, 2, 3) == (2, 1) and window_clamp(5, 2, 3) == (2, 2)               # P + Q >= n: the suffix gives way
    for n in (1, 2, 7):
        for p, q in BAD_WINDOWS:
            cp, cq = window_clamp(n, p, q)
            assert 0 <= cp <= n - 1 and 0 <= cq <= n - 1 - cp and n - cp - cq >= 1
    # whole rows: the window never leaves the utterance's own (clamped) rows, whatever the offsets hold
    cu, S = [0, 5, 6, 15], 15
    assert window_of(cu, S, 0, 1, 2) == (1, 3) and window_of(cu, S, 1, 0, 0) == (5, 6) and window_of(cu, S, 2, 8, 0) == (14, 15)
    for cu_bad in ([0, 5, 6, 15], [-4, 5, 3, 99], [20, 20, 20, 20]):
        for b in range(3):
            for p, q in BAD_WINDOWS:
                lo, hi = window_of(cu_bad, S, b, p, q)
                r0 = min(max(cu_bad[b], 0), S - 1)
                assert r0 <= lo < hi <= min(max(cu_bad[b + 1], r0 + 1), S)


def _bare_generator(cfg):
    sg = object.__new__(SpeechGenerator)                          # no device: only what runs before the first GPU call
    sg.ditto_model = types.SimpleNamespace(cfg=cfg)
    return sg


def test_argument_refusals():
    sg = _bare_generator(DiTTOConfig(256, 2, 4, 256, 256, 50))
    audio, text = torch.zeros(15, 256), torch.zeros(9, 256)
    packed = (text, [0, 3, 6, 9], audio, [0, 5, 6, 15])
    with pytest.raises(NotImplementedError, match="windowed"):
        sg.sample_guided_packed(*packed, suffix_lengths=[1, 0, 2], guidance=2.0, null_text_emb=text, guidance_rescale=0.5)
    with pytest.raises(ValueError, match="utterance 1"):          # validated before anything reaches the device
        sg.sample_guided_packed(*packed, suffix_lengths=[1, 1, 2])
    with pytest.raises(ValueError, match="utterance 2"):
        sg.sample_guided_packed(*packed, prompt_lengths=[0, 0, 5], suffix_lengths=[0, 0, 4])
    padded = (torch.zeros(1, 3, 256), torch.zeros(1, 5, 256))
    for entry in (sg.sample_guided, sg.sample_latents_strided):
        with pytest.raises(NotImplementedError, match="sample_guided_packed"):
            entry(*padded, suffix_lengths=[1])
    from ditto_tts_amd.dist import sample_sharded
    with pytest.raises(NotImplementedError, match="infilling"):
        sample_sharded(None, None, None, (), (), "cpu", suffix_lengths=[1])
    # fp8 linears and head_dim != 64 have no packed batches at all: refused like prompts
    for cfg in (DiTTOConfig(256, 2, 2, 256, 256, 50), ):
        with pytest.raises(NotImplementedError):
            _bare_generator(cfg).sample_guided_packed(*packed, suffix_lengths=[1, 0, 2])


def test_new_symbols_and_their_refusals():
    lib = hip.lib()
    names = declared_functions()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in hip.SYMBOLS
    assert lib.ditto_abi_version() == 10
    co = hip.MultistepCoef(1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    P = PTR
    # suffix_len is required; prompt_len may be NULL (those calls fail a later check: nothing here is ever launched)
    assert lib.ditto_guided_update_packed_window(P, P, None, None, 0, P, P, P, P, P, P, None, 2, 128, 64, 256, 1, None) == hip.ERR_ARG
    assert b"suffix_len" in lib.ditto_last_error()
    assert lib.ditto_guided_update_packed_tags_window(P, P, None, None, P, P, P, P, P, P, P, None, 2, 128, 64, 256, 1, None) == hip.ERR_ARG
    assert lib.ditto_guided_update_packed_window(P, P, None, None, 0, P, P, P, P, None, None, P, 2, 128, 64, 256, 1, None) == hip.ERR_ARG
    assert lib.ditto_guided_update_packed_window(P, P, None, None, 0, P, P, P, P, P, None, P, 2, 128, 64, 96, 1, None) == hip.ERR_SHAPE
    assert lib.ditto_guided_update_packed_tags_window(P, P, None, P, None, P, P, P, P, P, None, P, 2, 128, 64, 256, 1, None) == hip.ERR_ARG
    assert b"tags" in lib.ditto_last_error()
    assert lib.ditto_multistep_update_window(P, P, P, C.byref(co), None, P, P, None, None, 2, 128, 64, 256, 1, None) == hip.ERR_ARG
    assert b"suffix_len" in lib.ditto_last_error()
    assert lib.ditto_multistep_update_window(P, P, None, C.byref(co), None, P, P, None, P, 2, 128, 64, 256, 1, None) == hip.ERR_ARG
    assert lib.ditto_multistep_update_window(P, P, P, None, None, P, P, None, P, 2, 128, 64, 256, 1, None) == hip.ERR_ARG
    assert b"exactly one" in lib.ditto_last_error()
    assert lib.ditto_multistep_update_window(P, P, P, C.byref(co), None, P, P, None, P, 0, 128, 64, 256, 1, None) == hip.ERR_SHAPE
    assert lib.ditto_span_noise_window(P, P, None, 0, P, P, P, None, None, P, 2, 128, 64, 256, None) == hip.ERR_ARG
    assert lib.ditto_span_noise_window(P, P, P, 0, P, P, P, None, P, P, 2, 128, 64, 256, None) == hip.ERR_ARG
    assert b"exactly one" in lib.ditto_last_error()
    assert lib.ditto_span_noise_window(P, P, None, 0, None, P, P, None, P, P, 2, 128, 64, 256, None) == hip.ERR_ARG
    assert lib.ditto_span_mse_window(P, P, None, 0, P, None, None, 64, P, P, P, 1 << 20, 2, 128, 64, 256, None) == hip.ERR_ARG
    assert lib.ditto_span_mse_window(P, P, None, 0, P, None, P, 0, P, P, P, 1 << 20, 2, 128, 64, 256, None) == hip.ERR_SHAPE
    assert lib.ditto_span_mse_window(P, P, None, 0, P, None, P, 64, P, P, P, 4, 2, 128, 64, 256, None) == hip.ERR_SIZE
    assert lib.ditto_span_mse_window(P, P, None, 0, P, None, P, 64, P, None, P, 1 << 20, 2, 128, 64, 256, None) == hip.ERR_ARG
    # the step entries: a NULL model, and a NULL suffix_len
    assert lib.ditto_guided_step_packed_window_opts(None, P, P, P, P, P, None, P, None, None, 0, P, P, P, P, 2, 128, 64, 8, 8, 1, P, P, P,
                                                    1 << 20, None, None) == hip.ERR_ARG
    assert lib.ditto_guided_step_packed_tags_window_opts(None, P, P, P, P, P, None, P, None, None, None, P, P, P, P, 2, 128, 64, 8, 8, 1, P,
                                                         P, P, 1 << 20, None, None) == hip.ERR_ARG
    assert lib.ditto_guided_step_packed_multistep_window_opts(None, P, P, P, P, P, None, P, P, C.byref(co), None, P, 2, 128, 64, 8, 8, 1,
                                                              P, P, P, 1 << 20, None, None) == hip.ERR_ARG


def _req(row, P, n_frames, Q, x_T=None):
    return types.SimpleNamespace(row=row, P=P, n_frames=n_frames, Q=Q, rows=P + n_frames + Q, x_T=x_T)


def test_segments_of_a_suffixed_request():
    d4, dup = D // 4, 1000 * (D // 4)
    copy, draw = hip.REGROUP_COPY, hip.REGROUP_DRAW
    # a newcomer with prefix and suffix, x_T drawn: staged [prompt 40 | suffix 25] at row 10 of the x_T buffer
    r = _req(None, 40, 100, 25)
    assert staged_rows(r) == 65
    assert speech_segments(r, True, 2, 300, 10, d4, dup) == [
        [copy, _SRC_XT, _DST_X, 0, 10 * d4, 300 * d4, 40 * d4, dup],
        [draw, 0, _DST_X, 2, 0, 340 * d4, 100 * d4, dup],                  # n_frames d / 4 units, counted from 0, behind the prompt
        [copy, _SRC_XT, _DST_X, 0, 50 * d4, 440 * d4, 25 * d4, dup]]
    # its own x_T: staged [prompt | x_T | suffix]
    r = _req(None, 40, 100, 25, x_T=object())
    assert staged_rows(r) == 165
    assert speech_segments(r, True, 0, 0, 10, d4, 0) == [
        [copy, _SRC_XT, _DST_X, 0, 10 * d4, 0, 40 * d4, 0],
        [copy, _SRC_XT, _DST_X, 0, 50 * d4, 40 * d4, 100 * d4, 0],
        [copy, _SRC_XT, _DST_X, 0, 150 * d4, 140 * d4, 25 * d4, 0]]
    # a suffix only
    r = _req(None, 0, 64, 7)
    assert speech_segments(r, True, 1, 20, 0, d4, dup) == [[draw, 0, _DST_X, 1, 0, 20 * d4, 64 * d4, dup],
                                                           [copy, _SRC_XT, _DST_X, 0, 0, 84 * d4, 7 * d4, dup]]
    # no suffix: the segments of before (a record without the field included)
    plain = types.SimpleNamespace(row=None, P=40, n_frames=100, rows=140, x_T=None)
    assert speech_segments(plain, True, 0, 0, 0, d4, dup) == speech_segments(_req(None, 40, 100, 0), True, 0, 0, 0, d4, dup)
    assert len(speech_segments(plain, True, 0, 0, 0, d4, dup)) == 2 and staged_rows(plain) == 40
    # a survivor moves as one range, both contexts included; its history and its retirement cover the generated rows only
    r = _req(204, 40, 100, 25)
    assert speech_segments(r, False, 1, 140, 0, d4, dup) == [[copy, _SRC_X, _DST_X, 0, 204 * d4, 140 * d4, 165 * d4, dup]]
    assert history_segment(r, 140, d4) == [copy, _SRC_Q, _DST_Q, 0, 244 * d4, 180 * d4, 100 * d4, 0]
    r2 = _req(0, 0, 64, 7)
    assert retire_segments([r2, r], d4) == [[copy, _SRC_X, _DST_OUT, 0, 0, 0, 64 * d4, 0],
                                            [copy, _SRC_X, _DST_OUT, 0, 244 * d4, 64 * d4, 100 * d4, 0]]


@pytest.mark.parametrize("maxB", [1, 3, 8, 33])
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("multistep", [True, False])
def test_step_block_keyword_off_is_the_old_layout_and_on_appends(maxB, guided, multistep):
    off = step_block_layout(maxB, guided, multistep)
    assert step_block_layout(maxB, guided, multistep, infill=False) == off and "suffix" not in off
    # the layout of before, restated: ... | coef | phi, the block ending one field behind phi
    assert off["bytes"] == off["phi"] + off["f_stride"]
    assert set(off) == {"t", "seeds", "f_stride", "a", "ce", "cz", "w", "tags", "prompt", "partner", "coef", "phi", "bytes"}
    on = step_block_layout(maxB, guided, multistep, infill=True)
    for k, v in off.items():
        if k != "bytes":
            assert on[k] == v, k
    assert on["suffix"] == off["bytes"] and on["bytes"] == off["bytes"] + off["f_stride"]
    assert on["suffix"] % 16 == 0 and on["f_stride"] >= 4 * maxB


def _stream(infill, solver="ddim", guided=True):
    return GuidedStream(StubBatch(), _acp(), guided=guided, text_dim=TEXT_DIM, hidden_dim=D, max_rows=512, max_utterances=3,
                        max_text_rows=4096, solver=solver, infill=infill)


def test_stream_refusals_and_row_accounting():
    text, null = torch.zeros(4, TEXT_DIM), torch.zeros(5, TEXT_DIM)
    kw = dict(seed=1, guidance=2.0, null_text_emb=null, n_steps=4)
    plain = _stream(False)
    with pytest.raises(ValueError, match="infill=True"):
        plain.submit(text, 64, suffix=torch.zeros(8, D), **kw)
    assert plain.pending == 0
    plain.submit(text, 64, guidance_interval=(0, 49), **kw)              # a stream without the flag is the stream of before
    plain.submit(text, 64, guidance_rescale=0.5, **kw)
    for solver in ("ddim", "dpmpp2m"):
        s = _stream(True, solver)
        with pytest.raises(NotImplementedError, match="windowed"):
            s.submit(text, 64, guidance_interval=(0, 49), **kw)
        with pytest.raises(NotImplementedError, match="windowed"):
            s.submit(text, 64, guidance_rescale=0.5, **kw)
        for bad in (torch.zeros(0, D), torch.zeros(8, D + 1), torch.zeros(8), torch.zeros(8, D, dtype=torch.int32), [[0.0] * D]):
            with pytest.raises(ValueError, match="suffix"):
                s.submit(text, 64, suffix=bad, **kw)
        with pytest.raises(ValueError, match="never fit"):               # P + n_frames + Q against max_rows
            s.submit(text, 400, prompt=torch.zeros(60, D), suffix=torch.zeros(53, D), **kw)
        assert s.pending == 0
        # n_frames stays the generated frames; the request occupies P + n_frames + Q rows
        s.submit(text, 100, prompt=torch.zeros(40, D), suffix=torch.zeros(25, D), **kw)
        s.submit(text, 64, suffix=torch.zeros(7, D), **kw)
        s.submit(text, 300, **kw)                                        # 165 + 71 + 300 > 512: waits
        s.step()
        a = s.batch.steps[-1]
        assert (a.B, a.S, a.max_N) == (2, 236, 165) and a.prompt == [40, 0] and a.suffix == [25, 7]
        assert s.batch.regroups[-1][3] == [0, 165, 236] and s.pending == 1
        done = s.drain()
        assert sorted(h.id for h, _ in done) == [0, 1, 2]
        assert [x.suffix for x in s.batch.steps[-2:]] == [[0], [0]]       # the plain request alone at the end
