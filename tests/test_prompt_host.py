"""Speech prompts, the host side (no GPU): prompt_lengths validation, the refusals of the layouts that have no prompts, the stream's
admission arithmetic over P + n_frames rows, the segment table of a prompted newcomer / survivor / retiree in 16-byte units, and the
new entries in the header, the library and hip.py."""
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.serving import (_DST_OUT, _DST_X, _SRC_X, _SRC_XT, GuidedStream, Plan, retire_segments, speech_segments,
                                   staged_rows)
from ditto_tts_amd.varlen import validate_prompt_lengths
from test_stream_host import D, TEXT_DIM, StubBatch, _acp

NEW = ["ditto_guided_update_packed_prompt", "ditto_guided_update_packed_tags_prompt", "ditto_guided_step_packed_prompt_opts",
       "ditto_guided_step_packed_tags_prompt_opts", "ditto_span_noise_packed", "ditto_span_mse_packed"]


def test_prompt_lengths_validation():
    cu = [0, 5, 6, 15]
    assert validate_prompt_lengths([0, 0, 8], cu).tolist() == [0, 0, 8]
    assert validate_prompt_lengths(torch.tensor([4, 0, 0]), cu).dtype == torch.int32
    with pytest.raises(ValueError, match="utterance 1"):
        validate_prompt_lengths([0, 1, 0], cu)                   # a one-row utterance has no room for a prompt
    with pytest.raises(ValueError, match="utterance 0"):
        validate_prompt_lengths([5, 0, 0], cu)                   # P_b = N_b: nothing left to generate
    with pytest.raises(ValueError, match="utterance 2"):
        validate_prompt_lengths([0, 0, -1], cu)
    for bad in ([0, 0], [0, 0, 0, 0], [0.0, 0, 0], [True, 0, 0], torch.tensor([0.0, 0, 0]), torch.tensor([[0, 0, 0]]), 3, None):
        with pytest.raises(ValueError):
            validate_prompt_lengths(bad, cu)


def _bare_generator(cfg):
    sg = object.__new__(SpeechGenerator)                          # no device: only what runs before the first GPU call
    sg.ditto_model = types.SimpleNamespace(cfg=cfg)
    return sg


def test_sample_guided_packed_validates_before_any_launch_and_other_layouts_refuse():
    cfg = DiTTOConfig(256, 2, 4, 256, 256, 50)
    sg = _bare_generator(cfg)
    audio, text = torch.zeros(15, 256), torch.zeros(9, 256)
    with pytest.raises(ValueError, match="utterance 1"):
        sg.sample_guided_packed(text, [0, 3, 6, 9], audio, [0, 5, 6, 15], prompt_lengths=[0, 1, 0])
    with pytest.raises(ValueError, match=r"shape \[3\]"):
        sg.sample_guided_packed(text, [0, 3, 6, 9], audio, [0, 5, 6, 15], prompt_lengths=[0, 0])
    with pytest.raises(NotImplementedError, match="sample_guided_packed"):
        sg.sample_guided(torch.zeros(1, 3, 256), torch.zeros(1, 5, 256), prompt_lengths=[2])
    with pytest.raises(NotImplementedError, match="sample_guided_packed"):
        sg.sample_latents_strided(torch.zeros(1, 3, 256), torch.zeros(1, 5, 256), prompt_lengths=[2])
    from ditto_tts_amd.dist import sample_sharded
    with pytest.raises(NotImplementedError, match="prompts"):
        sample_sharded(None, None, None, None, None, "cpu", prompt_lengths=[2])
    # fp8 linears and head_dim != 64 refuse as packed batches do
    for bad in (DiTTOConfig(256, 2, 2, 256, 256, 50), DiTTOConfig(256, 2, 4, 256, 256, 50, fp8_linear=True)):
        with pytest.raises(NotImplementedError):
            _bare_generator(bad).sample_guided_packed(text, [0, 9], audio, [0, 15], prompt_lengths=[3])


def _stream(**kw):
    caps = dict(max_rows=512, max_utterances=3, max_text_rows=4096)
    caps.update(kw)
    return GuidedStream(StubBatch(), _acp(), guided=True, text_dim=TEXT_DIM, hidden_dim=D, **caps)


def _submit(s, n_frames, P=0, x_T=False, n_steps=2, **kw):
    return s.submit(torch.zeros(8, TEXT_DIM), n_frames, seed=7, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=n_steps,
                    prompt=torch.ones(P, D) if P else None, x_T=torch.zeros(n_frames, D) if x_T else None, **kw)


def test_submit_validates_the_prompt_and_counts_it_against_max_rows():
    s = _stream()
    for bad in (torch.zeros(0, D), torch.zeros(4, D + 1), torch.zeros(4, D, dtype=torch.long), torch.zeros(D), [[0.0] * D]):
        with pytest.raises(ValueError, match="prompt"):
            s.submit(torch.zeros(8, TEXT_DIM), 64, seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), prompt=bad)
    with pytest.raises(ValueError, match="max_rows"):
        _submit(s, 400, P=113)                                   # 513 rows can never fit 512
    with pytest.raises(ValueError, match="x_T"):                 # x_T stays [n_frames, d]: not [P + n_frames, d]
        s.submit(torch.zeros(8, TEXT_DIM), 64, seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), prompt=torch.zeros(4, D),
                 x_T=torch.zeros(68, D))
    assert s.pending == 0
    _submit(s, 400, P=112)                                       # 512: fits exactly


def test_admission_counts_prompt_plus_frames():
    s = _stream(max_rows=300)
    _submit(s, 100, P=100)                                       # 200 rows
    _submit(s, 60, P=50)                                         # 110 more: 310 > 300, waits although 100 + 60 frames would fit
    _submit(s, 50)
    s.step()
    a = s.batch.steps[-1]
    assert [x.id for x in a.handles] == [0] and (a.S, a.max_N, a.prompt) == (200, 200, [100])
    assert s.batch.regroups[-1][3] == [0, 200]
    s.step()                                                     # request 0 retires after its 2 steps
    s.step()
    a = s.batch.steps[-1]
    assert [x.id for x in a.handles] == [1, 2] and (a.S, a.max_N, a.prompt) == (160, 110, [50, 0])
    assert s.batch.regroups[-1][3] == [0, 110, 160]


def test_segment_tables_of_prompted_newcomers_survivors_and_retirees():
    s = _stream()
    _submit(s, 100, P=40, n_steps=3)                             # drawn x_T behind a prompt
    _submit(s, 64, P=0, n_steps=1)                               # no prompt: one draw segment, as before
    _submit(s, 90, P=30, x_T=True, n_steps=3)                    # its own x_T behind a prompt
    r0, r1, r2 = list(s._queue)
    s.step()
    plan = Plan([r0, r1, r2], [r0, r1, r2], True)
    assert plan.cu == [0, 140, 204, 324]
    d4 = D // 4
    dup = 324 * d4
    copy, draw = hip.REGROUP_COPY, hip.REGROUP_DRAW
    # newcomers (rows are those the stub regroup left: r.row = plan.cu[j]); the staging buffer holds [prompt0 | prompt2 | x_T2]
    assert speech_segments(r0, True, 0, 0, 0, d4, dup) == [[copy, _SRC_XT, _DST_X, 0, 0, 0, 40 * d4, dup],
                                                          [draw, 0, _DST_X, 0, 0, 40 * d4, 100 * d4, dup]]
    assert staged_rows(r0) == 40 and staged_rows(r1) == 0 and staged_rows(r2) == 120
    assert speech_segments(r1, True, 1, 140, 40, d4, dup) == [[draw, 0, _DST_X, 1, 0, 140 * d4, 64 * d4, dup]]
    assert speech_segments(r2, True, 2, 204, 40, d4, dup) == [[copy, _SRC_XT, _DST_X, 0, 40 * d4, 204 * d4, 30 * d4, dup],
                                                             [copy, _SRC_XT, _DST_X, 0, 70 * d4, 234 * d4, 90 * d4, dup]]
    # unguided: no duplicate half
    assert speech_segments(r0, True, 0, 0, 0, d4, 0)[1] == [draw, 0, _DST_X, 0, 0, 40 * d4, 100 * d4, 0]
    # r1 has retired after the first step; the survivors move as one range each, prompt included
    assert (r0.row, r2.row) == (0, 204)
    assert speech_segments(r2, False, 1, 140, 0, d4, 260 * d4) == [[copy, _SRC_X, _DST_X, 0, 204 * d4, 140 * d4, 120 * d4, 260 * d4]]
    # retirees: the generated rows only, one behind the other
    assert retire_segments([r0, r2], d4) == [[copy, _SRC_X, _DST_OUT, 0, 40 * d4, 0, 100 * d4, 0],
                                            [copy, _SRC_X, _DST_OUT, 0, 234 * d4, 100 * d4, 90 * d4, 0]]


def test_new_symbols_in_header_library_and_binding():
    txt = open(os.path.join(ROOT, "include", "ditto_hip.h")).read()
    lib = hip.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, txt), f"{name} is not declared in ditto_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in hip.SYMBOLS
    # the prompt entries are the existing signatures plus one pointer (prompt_len)
    for new, old in (("ditto_guided_update_packed_prompt", "ditto_guided_update_packed"),
                     ("ditto_guided_update_packed_tags_prompt", "ditto_guided_update_packed_tags"),
                     ("ditto_guided_step_packed_prompt_opts", "ditto_guided_step_packed_opts"),
                     ("ditto_guided_step_packed_tags_prompt_opts", "ditto_guided_step_packed_tags_opts")):
        assert len(hip.SYMBOLS[new][1]) == len(hip.SYMBOLS[old][1]) + 1
    assert lib.ditto_abi_version() == 10
    # null pointers are refused, not dereferenced
    assert lib.ditto_span_noise_packed(None, None, None, 0, None, None, None, None, None, 1, 1, 1, 64, None) == hip.ERR_ARG
    assert lib.ditto_span_mse_packed(None, None, None, 0, None, None, 64, None, None, None, 0, 1, 1, 1, 64, None) == hip.ERR_ARG
    assert lib.ditto_guided_update_packed_prompt(None, None, None, None, 0, None, None, None, None, None, None, 1, 1, 1, 64, 0,
                                                 None) == hip.ERR_ARG
