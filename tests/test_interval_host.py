"""Guidance in a limited interval on the host (no GPU): which steps of both schedules an interval guides, at its edges; the argument
validation and refusals of sample_guided_packed(guidance_interval=) and GuidedStream.submit(guidance_interval=); the stream's plan
for a step whose guided set G is a part of the batch — partner table, offsets [cu; S + cu_G[1:]], where the null conditioning of
members inside and outside G goes, the segments of an utterance entering G and of one leaving it, the segment count within the
table — and the new symbols."""
import types

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.sampler import SpeechGenerator, guided_steps, multistep_schedule, strided_schedule, validate_guidance_interval
from ditto_tts_amd.serving import _DST_COND, _DST_X, _SRC_COND, _SRC_NEW_COND, _SRC_X, GuidedStream, Plan, partner_table, regroup_table
from test_cabi_symbols import declared_functions
from test_stream_host import TEXT_DIM, D, StubBatch, _acp

NEW = ("ditto_guided_update_packed_mixed", "ditto_guided_step_packed_mixed_opts")
P = 4096   # a non-NULL pointer value: every call below fails its argument checks before anything touches it


# ---------------------------------------------------------------------------------------------------------------- the guided set
@pytest.mark.parametrize("schedule", [lambda ac, n: strided_schedule(ac, n, 0.0), multistep_schedule], ids=["ddim", "dpmpp2m"])
def test_guided_steps_at_the_edges(schedule):
    sched = schedule(_acp(), 6)
    taus = [row[0] for row in sched]
    assert taus == [49, 41, 32, 24, 16, 7]
    assert guided_steps(sched, None) == [True] * 6
    assert guided_steps(sched, (0, 49)) == [True] * 6                       # every step
    assert guided_steps(sched, (7, 49)) == [True] * 6                       # (the bounds are inclusive)
    assert guided_steps(sched, (36, 36)) == [False] * 6                     # t_lo = t_hi between two timesteps: no step
    assert guided_steps(sched, (8, 15)) == [False] * 6
    assert guided_steps(sched, (42, 49)) == [True] + [False] * 5            # only the first step
    assert guided_steps(sched, (49, 49)) == [True] + [False] * 5
    assert guided_steps(sched, (0, 15)) == [False] * 5 + [True]             # only the last step
    assert guided_steps(sched, (7, 7)) == [False] * 5 + [True]
    assert guided_steps(sched, (10, 35)) == [False, False, True, True, True, False]


def test_interval_validation():
    assert validate_guidance_interval(None, 50) is None
    assert validate_guidance_interval((0, 49), 50) == (0, 49) and validate_guidance_interval([3, 3], 50) == (3, 3)
    for bad in ((1.0, 5), (1, 5.5), (True, 5), "ab", (1, 2, 3), (5,), 7, (6, 5), (-1, 5), (0, 50), (50, 50)):
        with pytest.raises(ValueError, match="guidance_interval"):
            validate_guidance_interval(bad, 50)


def _bare_generator(cfg):
    sg = object.__new__(SpeechGenerator)                          # no device: only what runs before the first GPU call
    sg.ditto_model = types.SimpleNamespace(cfg=cfg)
    sg.betas = torch.zeros(cfg.diffusion_steps)
    return sg


def test_closed_call_refusals_before_any_launch():
    sg = _bare_generator(DiTTOConfig(256, 2, 4, 256, 256, 50))
    audio, text = torch.zeros(15, 256), torch.zeros(9, 256)
    packed = (text, [0, 3, 6, 9], audio, [0, 5, 6, 15])
    ok = dict(guidance=2.0, null_text_emb=text)
    for solver in ("ddim", "dpmpp2m"):
        for bad in ((1.5, 20), (20, 10), (0, 50), (-1, 4)):
            with pytest.raises(ValueError, match="guidance_interval"):
                sg.sample_guided_packed(*packed, solver=solver, guidance_interval=bad, **ok)
        with pytest.raises(ValueError, match="needs guidance"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_interval=(10, 35))
        with pytest.raises(ValueError, match="needs guidance"):
            sg.sample_guided_packed(*packed, solver=solver, guidance_interval=(10, 35), guidance=2.0)
    # the padded layouts do not get the argument
    padded = (torch.zeros(1, 3, 256), torch.zeros(1, 5, 256))
    for entry in (sg.sample_guided, sg.sample_latents_strided):
        with pytest.raises(TypeError, match="guidance_interval"):
            entry(*padded, guidance_interval=(10, 35))
    # the existing refusals stay: head_dim != 64 and fp8 linears before anything else of the packed path
    for cfg, word in ((DiTTOConfig(256, 2, 2, 256, 256, 50), "head_dim 64"), (DiTTOConfig(256, 2, 4, 256, 256, 50, fp8_linear=True), "fp8")):
        with pytest.raises(NotImplementedError, match=word):
            _bare_generator(cfg).sample_guided_packed(*packed, guidance_interval=(10, 35), **ok)


# ---------------------------------------------------------------------------------------------------------------- the stream
def _stream(guided=True, solver="ddim", **caps):
    kw = dict(max_rows=512, max_utterances=3, max_text_rows=4096)
    kw.update(caps)
    return GuidedStream(StubBatch(), _acp(), guided=guided, text_dim=TEXT_DIM, hidden_dim=D, solver=solver, **kw)


def _submit(s, frames, T, n_steps, interval, seed=1, **kw):
    return s.submit(torch.zeros(T, TEXT_DIM), frames, seed=seed, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=n_steps,
                    guidance_interval=interval, **kw)


def test_submit_refusals():
    s = _stream()
    for bad in ((1.5, 20), (20, 10), (0, 50), (-1, 4), "xy"):
        with pytest.raises(ValueError, match="guidance_interval"):
            _submit(s, 64, 8, 4, bad)
    assert s.pending == 0
    with pytest.raises(NotImplementedError, match="ddim"):
        _submit(_stream(solver="dpmpp2m"), 64, 8, 4, (10, 35))
    u = _stream(guided=False)
    with pytest.raises(ValueError, match="unguided"):
        u.submit(torch.zeros(8, TEXT_DIM), 64, seed=1, n_steps=4, guidance_interval=(10, 35))
    assert u.pending == 0
    _submit(s, 64, 8, 4, (10, 35))
    _submit(_stream(solver="dpmpp2m"), 64, 8, 4, None)
    assert s.pending == 1


def test_partner_table():
    assert partner_table([False, True, False, True]) == [-1, 0, -1, 1]
    assert partner_table([True] * 3) == [0, 1, 2] and partner_table([False] * 2) == [-1, -1] and partner_table([]) == []


def test_stream_follows_every_requests_interval_and_regroups_when_the_guided_set_changes():
    """requests 0 (6 steps, guided at its steps 2, 3, 4), 1 (3 steps, no interval) and 2 (4 steps: timesteps 49, 36, 24, 12; guided
    at its step 0 only), 2 submitted after step 1"""
    s = _stream()
    _submit(s, 70, 48, 6, (10, 35), seed=100)
    _submit(s, 64, 20, 3, None, seed=101)
    steps = 0
    while steps == 0 or s.pending or s.active:
        if steps == 1:
            _submit(s, 40, 7, 4, (45, 49), seed=102)
        s.step()
        steps += 1
    got = [([h.id for h in a.handles], a.partner, a.G, a.S_G) for a in s.batch.steps]
    assert got == [([0, 1], [-1, 0], 1, 64), ([0, 1, 2], [-1, 0, 1], 2, 104), ([0, 1, 2], [0, 1, -1], 2, 134),
                   ([0, 2], [0, -1], 1, 70), ([0, 2], [0, -1], 1, 70), ([0], [-1], 0, 0)]
    # a regroup at 1 (start), 2 (arrival), 3 (the guided set alone changes), 4 (retirement), 6 (retirement + G); none at 5
    assert [g[0] for g in s.batch.regroups] == [1, 2, 3, 4, 6]
    # an interval changes nothing a neighbour or the admission sees: the same S, S_T, t, coefficients and tags as without it
    p = _stream()
    for k, (n, t, st) in enumerate(((70, 48, 6), (64, 20, 3))):
        _submit(p, n, t, st, None, seed=100 + k)
    p.step()
    _submit(p, 40, 7, 4, None, seed=102)
    p.drain()
    for a, b in zip(s.batch.steps, p.batch.steps):
        for name in ("B", "S", "max_N", "S_T", "max_T", "t", "a", "ce", "cz", "w", "tags", "seeds", "prompt"):
            assert getattr(a, name) == getattr(b, name), name
    assert [a.G == a.B for a in p.batch.steps] == [True] * 6 and [g[0] for g in p.batch.regroups] == [1, 2, 4, 6]


def test_admission_counts_null_rows_whatever_the_interval():
    s = _stream(max_text_rows=60)
    kw = dict(guidance=1.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=1, guidance_interval=(0, 0))     # never guided
    s.submit(torch.zeros(30, TEXT_DIM), 64, seed=1, **kw)           # 35 conditioning rows
    s.submit(torch.zeros(25, TEXT_DIM), 64, seed=2, **kw)           # 30 more: 65 > 60
    s.step()
    assert [x.id for x in s.batch.steps[-1].handles] == [0] and s.batch.steps[-1].G == 0


def _member(k, rows, T, T_null, P=0, **where):
    r = types.SimpleNamespace(handle=types.SimpleNamespace(id=k), rows=rows, P=P, n_frames=rows - P, T=T, T_null=T_null, x_T=None)
    r.__dict__.update(where)
    return r


def test_plan_layout_and_the_segments_of_entering_and_leaving_the_guided_set():
    """three survivors of a batch in which 0 and 1 were guided and 2 was not (null conditioning parked); at the coming step 0 leaves
    the guided set, 1 stays, 2 enters it, and newcomer 3 arrives guided"""
    d4, kv16, tm16 = D // 4, 24, 8
    r0 = _member(0, 70, 48, 5, b=0, row=0, trow=0, nrow=75 + 0, ntm=3 + 0)
    r1 = _member(1, 64, 20, 6, b=1, row=70, trow=48, nrow=75 + 5, ntm=3 + 1)
    r2 = _member(2, 40, 7, 4, P=10, b=2, row=134, trow=68, nrow=75 + 11, ntm=3 + 2)
    r3 = _member(3, 30, 9, 3)
    plan = Plan([r0, r1, r2, r3], [r3], True, [False, True, True, True])
    S, Tt = 204, 84
    assert plan.cu == [0, 70, 134, 174, 204] and plan.partner == [-1, 0, 1, 2] and plan.cu_g == [0, 64, 104, 134]
    assert plan.offsets == [0, 70, 134, 174, 204, 204 + 64, 204 + 104, 204 + 134]                 # [cu; S + cu_G[1:]]
    assert plan.text_offsets == [0, 48, 68, 75, 84, 84 + 6, 84 + 10, 84 + 13]
    assert plan.null_row == [13, 0, 6, 10] and plan.null_tm == [3, 0, 1, 2]                      # G's first, 0's parked behind them
    assert plan.cu_null == [0, 5, 11, 15, 18]
    everyone = Plan([r0, r1, r2, r3], [r3], True)                                                # the default: today's layout
    assert everyone.offsets == plan.cu + [S + c for c in plan.cu[1:]] and everyone.partner == [0, 1, 2, 3]
    assert everyone.null_row == everyone.cu_null[:-1] and everyone.null_tm == [0, 1, 2, 3]
    assert everyone.text_offsets == plan.cu_text + [Tt + c for c in everyone.cu_null[1:]]
    segs, tail = regroup_table(plan, d4=d4, kv16=kv16, tm16=tm16, tmod_old16=5000, tmod_new16=6000, new_image={3: (7000, 7400)},
                               multistep=False, cu_pad=12)
    copy, draw = hip.REGROUP_COPY, hip.REGROUP_DRAW
    by = lambda k: segs[5 * k:5 * k + 5]                  # five segments per member here: its rows, then its conditioning
    # 0 leaves G: its rows move as one range with no unconditional copy; its null K/V and tmod are parked behind G's
    assert by(0) == [[copy, _SRC_X, _DST_X, 0, 0, 0, 70 * d4, 0],
                     [copy, _SRC_COND, _DST_COND, 0, 0, 0, 48 * kv16, 0], [copy, _SRC_COND, _DST_COND, 0, 5000, 6000, tm16, 0],
                     [copy, _SRC_COND, _DST_COND, 0, 75 * kv16, (Tt + 13) * kv16, 5 * kv16, 0],
                     [copy, _SRC_COND, _DST_COND, 0, 5000 + 3 * tm16, 6000 + (4 + 3) * tm16, tm16, 0]]
    # 1 stays: copy 0, at row S + 0
    assert by(1)[0] == [copy, _SRC_X, _DST_X, 0, 70 * d4, 70 * d4, 64 * d4, (S - 70) * d4]
    assert by(1)[3] == [copy, _SRC_COND, _DST_COND, 0, 80 * kv16, Tt * kv16, 6 * kv16, 0]
    # 2 enters G: the copy comes from its conditional rows through dup_off (prompt included), its parked null conditioning moves
    # where the forward reads it
    assert by(2) == [[copy, _SRC_X, _DST_X, 0, 134 * d4, 134 * d4, 40 * d4, (S + 64 - 134) * d4],
                     [copy, _SRC_COND, _DST_COND, 0, 68 * kv16, 68 * kv16, 7 * kv16, 0],
                     [copy, _SRC_COND, _DST_COND, 0, 5000 + 2 * tm16, 6000 + 2 * tm16, tm16, 0],
                     [copy, _SRC_COND, _DST_COND, 0, 86 * kv16, (Tt + 6) * kv16, 4 * kv16, 0],
                     [copy, _SRC_COND, _DST_COND, 0, 5000 + 5 * tm16, 6000 + (4 + 1) * tm16, tm16, 0]]
    # the newcomer: drawn x_T with its copy, conditioning from its own image
    assert by(3) == [[draw, 0, _DST_X, 3, 0, 174 * d4, 30 * d4, (S + 104 - 174) * d4],
                     [copy, _SRC_NEW_COND, _DST_COND, 0, 7000, 75 * kv16, 9 * kv16, 0],
                     [copy, _SRC_NEW_COND, _DST_COND, 0, 7400, 6000 + 3 * tm16, tm16, 0],
                     [copy, _SRC_NEW_COND, _DST_COND, 0, 7000 + 9 * kv16, (Tt + 10) * kv16, 3 * kv16, 0],
                     [copy, _SRC_NEW_COND, _DST_COND, 0, 7400 + tm16, 6000 + (4 + 2) * tm16, tm16, 0]]
    assert tail[:8].tolist() == plan.offsets and tail[12:20].tolist() == plan.text_offsets and len(tail) == 24
    # the destinations of the null conditioning tile [Tt, Tt + 18) and tmod rows [4, 8) exactly: nothing overlaps, nothing is lost
    null_kv = sorted((sg[5] // kv16 - Tt, sg[6] // kv16) for k in range(4) for sg in [by(k)[3]])
    assert null_kv == [(0, 6), (6, 4), (10, 3), (13, 5)]
    assert sorted((by(k)[4][5] - 6000) // tm16 for k in range(4)) == [4, 5, 6, 7]
    # the table holds it: at most 7 segments per member (prompt + x_T + history + 4 of conditioning) and the offsets
    assert len(segs) == 21 <= 8 * 4 + 8


def test_new_symbols_and_their_refusals():
    lib = hip.lib()
    names = declared_functions()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in hip.SYMBOLS
    assert lib.ditto_abi_version() == 10

    def upd(x2=P, eps2=P, noise=None, seeds=None, tags=None, w=P, cu=P, partner=P, B=4, G=2, S=128, S_G=64, max_N=64, d=256):
        return lib.ditto_guided_update_packed_mixed(x2, eps2, noise, seeds, tags, w, P, P, P, cu, partner, None, B, G, S, S_G, max_N, d, None)

    for kw, code, word in [(dict(x2=None), hip.ERR_ARG, b"null"), (dict(cu=None), hip.ERR_ARG, b"null"), (dict(partner=None), hip.ERR_ARG, b"null"),
                           (dict(w=None), hip.ERR_ARG, b"needs w"), (dict(seeds=P), hip.ERR_ARG, b"tags"),
                           (dict(noise=P, seeds=P, tags=P), hip.ERR_ARG, b"exclusive"), (dict(B=0), hip.ERR_SHAPE, b"positive"),
                           (dict(d=96), hip.ERR_SHAPE, b"% 64"), (dict(G=5), hip.ERR_SHAPE, b"G"), (dict(G=-1), hip.ERR_SHAPE, b"G"),
                           (dict(G=0), hip.ERR_SHAPE, b"S_G"), (dict(S_G=0), hip.ERR_SHAPE, b"S_G"), (dict(S_G=129), hip.ERR_SHAPE, b"S_G")]:
        assert upd(**kw) == code, kw
        assert word in lib.ditto_last_error(), (kw, lib.ditto_last_error())
    assert lib.ditto_guided_step_packed_mixed_opts(None, P, P, P, P, P, P, None, None, None, None, P, P, P, P, 4, 2, 128, 64, 64, 8, 8, P, P,
                                                   P, 1 << 20, None, None) == hip.ERR_ARG
