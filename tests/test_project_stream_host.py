"""Projected guidance in a request stream (GuidedStream(project=True), submit(guidance_projection=, ...)) on the host, against a stub
batch that records calls: include/ditto_project_stream.h is a seventh table beside the six there were; the step block only grows;
every refusal leaves the stream as it was; a request's per-step coefficient rows are sampler.project_table's for that utterance alone;
its step kinds are 3 / 1 / 0; the regroup table carries the direction of a projected survivor that has had a guided step and has one to
come, and of nobody else; and the three C entries refuse bad arguments before any launch.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ditto_tts_amd import hip
from ditto_tts_amd.sampler import guided_steps, multistep_schedule, multistep_schedule_v, project_table, projection_vectors, strided_schedule
from ditto_tts_amd.serving import (DeviceBatch, GuidedStream, Plan, Request, StreamHandle, direction_segment, regroup_table,
                                   step_block_layout)
from test_refresh_stream_host import D, TEXT_DIM, StubBatch, _acp

PROJECT1, UPDATE, STEP = ("ditto_guidance_project_packed_mixed", "ditto_guided_update_packed_project_mixed",
                          "ditto_guided_step_packed_project_mixed_opts")
NEW = (PROJECT1, UPDATE, STEP)
P = 4096   # a non-NULL, 256-byte aligned pointer value: every call below fails its argument checks before anything touches it


def _stream(project=True, **kw):
    caps = dict(max_rows=300, max_utterances=3, max_text_rows=4096, guided=True)
    caps.update(kw)
    return GuidedStream(StubBatch(), _acp(), text_dim=TEXT_DIM, hidden_dim=D, project=project, **caps)


OK = dict(seed=1, guidance=4.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=8, eta=1.0)
TEXT = torch.zeros(8, TEXT_DIM)


# ---------------------------------------------------------------- the table
def test_the_header_is_a_seventh_table_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ditto_project_stream.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ditto_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(NEW) == sorted(hip.PROJECT_STREAM_PROTOTYPES) == sorted(hip.PROJECT_STREAM_SYMBOLS)
    lib = hip.lib()
    for n in names:
        res, params = hip.PROJECT_STREAM_PROTOTYPES[n]
        fn = getattr(lib, n)
        assert fn.restype == res == C.c_int and list(fn.argtypes) == [t for _, t in params], n
        assert [p for p, _ in params] == list(hip._ORDER[n])
    # the other six tables: disjoint from the new names, and the sizes they had
    others = (hip.SYMBOLS, hip.OPTIM_SYMBOLS, hip.TRAIN_ROWS_SYMBOLS, hip.TEXT_GRAD_SYMBOLS, hip.REFRESH_SYMBOLS, hip.PROJECT_SYMBOLS)
    assert [len(t) for t in others] == [143, 4, 15, 4, 2, 6]
    for t in others:
        assert not set(NEW) & set(t)
    assert lib.ditto_abi_version() == 10
    # the arguments: the mixed entries' plus the projection's
    mixed = [p for p, _ in hip.PROTOTYPES["ditto_guided_step_packed_mixed_opts"][1]]
    assert sorted(p for p, _ in hip.PROJECT_STREAM_PROTOTYPES[STEP][1]) == sorted(mixed + ["kind", "dir", "proj", "scratch", "scratch_bytes"])
    upd = [p for p, _ in hip.PROTOTYPES["ditto_guided_update_packed_mixed"][1]]
    assert sorted(p for p, _ in hip.PROJECT_STREAM_PROTOTYPES[UPDATE][1]) == sorted(upd + ["kind", "dir", "pcoef"])
    assert [p for p, _ in hip.PROJECT_STREAM_PROTOTYPES[PROJECT1][1]] == [
        "x2", "eps2", "dir", "proj", "cu", "partner", "kind", "prompt_len", "B", "G", "S", "S_G", "max_N", "d", "scratch", "scratch_bytes",
        "stream"]
    assert (hip.KIND_PLAIN, hip.KIND_CFG, hip.KIND_PROJECT) == (0, 1, 3) and hip.KIND_REUSE == 2
    # hip.call's header rule names the new header for a misspelt mixed entry, and still ditto_project.h for a closed one
    with pytest.raises(TypeError, match=r"ditto_project_stream\.h declares no such entry"):
        hip.call("ditto_guided_update_packed_project_mixed_x")
    with pytest.raises(TypeError, match=r"ditto_project\.h declares no such entry"):
        hip.call("ditto_guided_update_packed_project_x")


# ---------------------------------------------------------------- the step block
@pytest.mark.parametrize("maxB", [1, 3, 4, 32, 33])
def test_step_block_without_project_is_unchanged_and_with_project_only_appends(maxB):
    pad = lambda n: (n + 15) // 16 * 16
    f = pad(4 * maxB)
    for multistep, infill, refresh in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        base = step_block_layout(maxB, True, multistep, infill, refresh)
        assert base == step_block_layout(maxB, True, multistep, infill, refresh, project=False) and "proj" not in base
        # the layout as it stood before the argument existed, field by field
        o_f = pad(16 * maxB) + pad(8 * maxB)
        want = {"t": 0, "seeds": pad(16 * maxB), "f_stride": f}
        for k, name in enumerate(("a", "ce", "cz", "w", "tags", "prompt", "partner", "coef")):
            want[name] = o_f + k * f
        want["phi"] = pad(want["coef"] + (32 * maxB if multistep else 0))
        want["bytes"] = want["phi"] + f
        for on, name in ((infill, "suffix"), (refresh, "kind")):
            if on:
                want[name], want["bytes"] = want["bytes"], want["bytes"] + f
        assert base == want
    base = step_block_layout(maxB, True, False)
    ext = step_block_layout(maxB, True, False, project=True)
    assert ext["kind"] == base["bytes"] and ext["proj"] == base["bytes"] + f and ext["proj"] % 16 == 0
    assert ext["bytes"] == ext["proj"] + 32 * maxB and C.sizeof(hip.ProjectCoef) == 32
    assert {k: v for k, v in ext.items() if k not in ("kind", "proj", "bytes")} == {k: v for k, v in base.items() if k != "bytes"}


# ---------------------------------------------------------------- refusals
def test_refusals_at_construction_and_submit_leave_the_stream_as_it_was():
    with pytest.raises(ValueError, match="guided"):
        _stream(guided=False)
    with pytest.raises(NotImplementedError, match="ddim"):
        _stream(solver="dpmpp2m")
    with pytest.raises(NotImplementedError, match="infill"):
        _stream(infill=True)
    with pytest.raises(NotImplementedError, match="refresh"):
        _stream(refresh=True)

    class Eng:                                                            # DeviceBatch refuses the same before it makes a buffer
        cfg = None

    for kw, err in ((dict(solver="dpmpp2m"), NotImplementedError), (dict(infill=True), NotImplementedError),
                    (dict(refresh=True), NotImplementedError), (dict(guided=False), ValueError)):
        args = dict(max_rows=64, max_utterances=1, max_text_rows=8, guided=True, project=True)
        args.update(kw)
        with pytest.raises(err):
            DeviceBatch(Eng(), **args)
    plain = _stream(project=False)
    for kw in (dict(guidance_projection=0.0), dict(guidance_norm_threshold=1.0), dict(guidance_momentum=-0.5),
               dict(guidance_projection=0.5, guidance_momentum=-0.5)):
        with pytest.raises(ValueError, match="project=True"):
            plain.submit(TEXT, 64, **kw, **OK)
    assert plain.pending == 0 and plain._next_id == 0
    s = _stream()
    # sampler.projection_vectors' ranges and errors
    for kw, word in ((dict(guidance_projection=1.5), "guidance_projection"), (dict(guidance_projection=-0.1), "guidance_projection"),
                     (dict(guidance_projection=True), "guidance_projection"), (dict(guidance_projection="0"), "guidance_projection"),
                     (dict(guidance_projection=[0.0, 0.0]), "guidance_projection"),
                     (dict(guidance_projection=0.0, guidance_norm_threshold=0.0), "guidance_norm_threshold"),
                     (dict(guidance_projection=0.0, guidance_norm_threshold=float("nan")), "guidance_norm_threshold"),
                     (dict(guidance_projection=0.0, guidance_momentum=1.0), "guidance_momentum"),
                     (dict(guidance_projection=0.0, guidance_momentum=-1.0), "guidance_momentum"),
                     (dict(guidance_norm_threshold=1.0), "needs guidance_projection"), (dict(guidance_momentum=0.5), "needs guidance_projection")):
        with pytest.raises(ValueError, match=word) as e:
            s.submit(TEXT, 64, **kw, **OK)
        with pytest.raises(ValueError) as want:                           # the closed call's validator gives the same error
            projection_vectors(kw.get("guidance_projection"), kw.get("guidance_norm_threshold"), kw.get("guidance_momentum"), 1)
        assert str(e.value) == str(want.value)
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        s.submit(TEXT, 64, guidance_rescale=0.5, **OK)
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        s.submit(TEXT, 64, guidance_projection=0.0, guidance_rescale=0.5, **OK)
    assert s.pending == 0 and s._next_id == 0
    s.submit(TEXT, 64, guidance_projection=0.0, guidance_rescale=0.0, **OK)       # phi = 0: no rescale at all
    s.submit(TEXT, 64, **OK)
    s.submit(TEXT, 64, guidance_projection=1.0, guidance_norm_threshold=2.0, guidance_momentum=-0.5, guidance_interval=(10, 40), **OK)
    assert s.pending == 3 and s._next_id == 3


# ---------------------------------------------------------------- per-request coefficients and kinds
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("interval", [None, (10, 40), (0, 20)])
def test_a_requests_coefficient_rows_are_project_table_for_one_utterance(interval, prediction):
    s = _stream(prediction=prediction)
    n_steps, w, apg = 8, 4.0, (0.25, 1.5, -0.5)
    s.submit(TEXT, 64, guidance_interval=interval, guidance_projection=apg[0], guidance_norm_threshold=apg[1], guidance_momentum=apg[2],
             **OK)
    s.submit(TEXT, 50, guidance_interval=interval, **OK)
    acp = _acp().double()
    flags = guided_steps(strided_schedule(acp, n_steps, 1.0), interval)
    x0 = (multistep_schedule_v if prediction == "v" else multistep_schedule)(acp, n_steps)
    want = project_table(projection_vectors(*apg, 1), torch.tensor([w]), x0, flags)[:, 0].numpy()
    assert want.shape == (n_steps, 8)
    use_prev = want.view(np.int32)[:, 6].tolist()
    first = flags.index(True)
    assert use_prev == [int(g and i > first) for i, g in enumerate(flags)]   # 1 from its second guided step on, interval-aware
    for i in range(n_steps):
        s.step()
        a = s.batch.steps[-1]
        assert a.kind == [hip.KIND_PROJECT if flags[i] else hip.KIND_PLAIN, hip.KIND_CFG if flags[i] else hip.KIND_PLAIN]
        assert a.in_g == [bool(flags[i])] * 2 and a.G == 2 * int(flags[i]) and a.S_G == (64 + 50) * int(flags[i])
        assert a.partner == ([0, 1] if flags[i] else [-1, -1])
        assert a.proj[1] is None and a.proj[0].dtype == np.float32
        assert a.proj[0].view(np.int32).tolist() == want[i].view(np.int32).tolist(), i      # bit for bit, use_prev included
    assert s.active == 0 and len(s._x0_rows) == 1                               # the x0 schedule is cached per n_steps


def _request(id_, frames, P=0, kinds=None, i=0, projected=True):
    r = Request(StreamHandle(id_), torch.zeros(8, TEXT_DIM), torch.zeros(5, TEXT_DIM), frames, id_, 2.0, len(kinds), 0.0, None, None,
                prompt=torch.zeros(P, D) if P else None, kinds=kinds, pcoef=np.zeros((len(kinds), 8), np.float32) if projected else None)
    r.i = i
    return r


# ---------------------------------------------------------------- the regroup table
def test_the_regroup_table_carries_the_direction_of_a_survivor_between_two_guided_steps_only():
    d4 = D // 4
    G, U = hip.KIND_REFRESH, hip.KIND_PLAIN                              # a request's own schedule: guided or not
    a = _request(0, 40, P=3, kinds=[G, G, G, G], i=2)                    # between guided steps: carried
    b = _request(1, 30, kinds=[U, U, G, G], i=2)                         # its first guided step is coming: nothing to carry
    c = _request(2, 20, P=2, kinds=[G, G, U, U], i=2)                    # no guided step to come: not carried
    e = _request(3, 25, kinds=[G, U, U, G], i=2)                         # guided, now outside its interval, guided again later: carried
    f = _request(4, 15, kinds=[G, G, G, G], i=2, projected=False)        # guided without a projection: it has no direction
    n = _request(5, 10, kinds=[G, G, G, G], i=0)                         # a newcomer
    assert [r.carries_direction() for r in (a, b, c, e, f, n)] == [True, False, False, True, False, False]
    assert [r.project_kind_now() for r in (a, b, c, e, f, n)] == [3, 3, 0, 0, 1, 3]
    members = [a, b, c, e, f, n]
    for j, (r, row) in enumerate(zip(members[:-1], (0, 50, 90, 120, 150))):       # where the survivors stand now (holes between them)
        r.b, r.row, r.trow, r.nrow, r.ntm = j, row, 8 * j, 60 + 5 * j, 6 + j
    in_g = [r.project_kind_now() != 0 for r in members]
    carry = [r is not n and r.carries_direction() for r in members]
    plan = Plan(members, [n], True, in_g, None, carry)
    kw = dict(d4=d4, kv16=64, tm16=32, tmod_old16=5000, tmod_new16=6000, new_image={5: (0, 900)}, multistep=False, cu_pad=16)
    segs, _ = regroup_table(plan, **kw)
    carried = [s for s in segs if s[1] == 5 and s[2] == 4]               # the history's slots: source 5, destination 4
    assert carried == [direction_segment(a, plan.cu[0], d4), direction_segment(e, plan.cu[3], d4)]
    assert carried[0] == [hip.REGROUP_COPY, 5, 4, 0, (0 + 3) * d4, (0 + 3) * d4, 40 * d4, 0]      # its generated rows, no duplicate
    assert carried[1] == [hip.REGROUP_COPY, 5, 4, 0, 120 * d4, plan.cu[3] * d4, 25 * d4, 0]
    # without a projection in the stream the table is the one it was
    plain = Plan(members, [n], True, in_g)
    segs3, _ = regroup_table(plain, **kw)
    assert plain.carry is None and segs3[:-1] == [s for s in segs if s not in carried][:-1] and len(segs3) == len(segs) - 2
    # a full batch of carried survivors with prompts still fits DeviceBatch's max_seg = 8 maxB + 8; so does one of newcomers
    maxB = 6
    full = [_request(k, 8, P=1, kinds=[G] * 4, i=1) for k in range(maxB)]
    for j, r in enumerate(full):
        r.b, r.row, r.trow, r.nrow, r.ntm = j, 9 * j, 8 * j, 100 + 5 * j, maxB + j
    segs4, _ = regroup_table(Plan(full, [], True, [True] * maxB, None, [True] * maxB), **{**kw, "new_image": {}})
    assert len(segs4) == 6 * maxB + 1 <= 8 * maxB + 8
    new = [_request(k, 8, P=1, kinds=[G] * 4) for k in range(maxB)]
    segs5, _ = regroup_table(Plan(new, new, True, [True] * maxB, None, [False] * maxB),
                             **{**kw, "new_image": {k: (100 * k, 100 * k + 50) for k in range(maxB)}})
    assert len(segs5) == 6 * maxB + 1 <= 8 * maxB + 8
    assert hip.REGROUP_BUFS == 6


def test_the_stream_names_the_carried_directions_and_regroups_when_the_guided_set_changes():
    s = _stream()
    apg = dict(guidance_projection=0.0, guidance_momentum=-0.5)
    s.submit(TEXT, 64, guidance_interval=(20, 40), **apg, **OK)           # timesteps 49 43 36 30 24 18 12 5: P P 3 3 3 P P P
    s.submit(TEXT, 50, **apg, **{**OK, "n_steps": 6})
    s.submit(TEXT, 40, **OK)
    while s.pending or s.active:
        s.step()
    carried = {n: plan.carry for n, plan in s.batch.regroups}
    # step 1 admits (newcomers carry nothing); step 3: request 0 enters the guided set — its first guided step, request 1 is between
    # two; step 6: request 0 leaves it for good; step 7: request 1 has left the batch after its 6 steps; the other two end with step 8
    assert sorted(carried) == [1, 3, 6, 7] and len(s.batch.steps) == 8
    assert carried[1] == [False] * 3 and carried[3] == [False, True, False] and carried[6] == [False, True, False]
    assert carried[7] == [False, False]
    for n, plan in s.batch.regroups:
        assert plan.kind is None and plan.in_g == s.batch.steps[n - 1].in_g == [k != 0 for k in s.batch.steps[n - 1].kind]
    # a stream made without project=True hands the batch no carry list, and the kinds it always did
    plain = _stream(project=False)
    plain.submit(TEXT, 64, **OK)
    plain.step()
    assert plain.batch.regroups[0][1].carry is None and plain.batch.steps[0].kind == [hip.KIND_REFRESH] and plain.batch.steps[0].proj is None


# ---------------------------------------------------------------- the C entries' argument checks
def _refused(name, base, cases):
    lib = hip.lib()
    for kw, code, word in cases:
        a = dict(base)
        a.update(kw)
        assert hip.call(name, **a) == code, (name, kw, lib.ditto_last_error())
        msg = lib.ditto_last_error()
        assert name.encode() in msg and word in msg, (name, kw, msg)


def test_the_entries_refuse_bad_arguments_before_any_launch():
    need = hip.lib().ditto_guidance_project_bytes(3, 9, 256)
    rows = dict(cu=P, partner=P, kind=P, prompt_len=None, B=3, G=2, S=15, S_G=12, max_N=9, d=256, stream=None)
    shared = [(dict(d=96), hip.ERR_SHAPE, b"% 64"), (dict(max_N=16), hip.ERR_SHAPE, b"max_N <= S"), (dict(B=0, G=0, S_G=0), hip.ERR_SHAPE, b"positive"),
              (dict(B=16), hip.ERR_SHAPE, b"at least one row"), (dict(G=4), hip.ERR_SHAPE, b"G <= B"), (dict(S_G=16), hip.ERR_SHAPE, b"S_G"),
              (dict(G=0), hip.ERR_SHAPE, b"S_G"), (dict(S_G=0), hip.ERR_SHAPE, b"S_G"), (dict(G=3, S_G=2), hip.ERR_SHAPE, b"S_G"),
              (dict(x2=None), hip.ERR_ARG, b"null"), (dict(eps2=None), hip.ERR_ARG, b"null"), (dict(dir=None), hip.ERR_ARG, b"null"),
              (dict(cu=None), hip.ERR_ARG, b"null"), (dict(partner=None), hip.ERR_ARG, b"null"), (dict(kind=None), hip.ERR_ARG, b"null"),
              (dict(x2=P + 4), hip.ERR_ARG, b"16-byte"), (dict(dir=P + 8), hip.ERR_ARG, b"16-byte")]
    _refused(PROJECT1, dict(x2=P, eps2=P, dir=P, proj=P, scratch=P, scratch_bytes=need, **rows), shared + [
        (dict(proj=None), hip.ERR_ARG, b"null"), (dict(scratch=None), hip.ERR_ARG, b"null"), (dict(proj=P + 8), hip.ERR_ARG, b"16-byte"),
        (dict(scratch=P + 16), hip.ERR_ARG, b"256-byte"), (dict(scratch_bytes=need - 1), hip.ERR_SIZE, b"ditto_guidance_project_bytes")])
    upd = dict(x2=P, eps2=P, dir=P, pcoef=P, noise=None, seeds=None, tags=None, w=P, a=P, ce=P, cz=P, **rows)
    _refused(UPDATE, upd, shared + [
        (dict(pcoef=None), hip.ERR_ARG, b"pcoef"), (dict(pcoef=P + 4), hip.ERR_ARG, b"pcoef"), (dict(noise=P, seeds=P, tags=P), hip.ERR_ARG, b"exclusive"),
        (dict(noise=P + 4), hip.ERR_ARG, b"16-byte"), (dict(a=None), hip.ERR_ARG, b"null a"), (dict(ce=None), hip.ERR_ARG, b"null a"),
        (dict(seeds=P, tags=P, cz=None), hip.ERR_ARG, b"null a"), (dict(w=None), hip.ERR_ARG, b"null w"), (dict(seeds=P), hip.ERR_ARG, b"tags")])
    # the step refuses a null model before anything else, naming itself
    params = [p for p, _ in hip.PROJECT_STREAM_PROTOTYPES[STEP][1]]
    args = {p: None for p in params}
    args.update(B=1, G=0, S=8, S_G=0, max_N=8, S_T=4, max_T=4, workspace_bytes=0, scratch_bytes=0)
    assert hip.call(STEP, **args) == hip.ERR_ARG and STEP.encode() in hip.lib().ditto_last_error()
