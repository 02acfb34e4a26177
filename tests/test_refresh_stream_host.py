"""Guidance reuse in a request stream (GuidedStream(refresh=True), submit(guidance_refresh=k)) on the host, against a stub batch that
records calls: every request's step kinds are sampler.refresh_plan of its own guided steps; a regroup runs exactly when the membership
or the refresh set changes; the step block only grows; the regroup table carries the direction of a survivor about to reuse and of
nobody else; every refusal; and the C entries of include/ditto_refresh.h refuse bad arguments before any launch.  No GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from ditto_tts_amd import hip
from ditto_tts_amd.sampler import guided_steps, refresh_plan, strided_schedule
from ditto_tts_amd.serving import (DeviceBatch, GuidedStream, Plan, Request, StreamHandle, direction_segment, regroup_table,
                                   step_block_layout)

TEXT_DIM, D = 32, 64
CODE = {"plain": hip.KIND_PLAIN, "refresh": hip.KIND_REFRESH, "reuse": hip.KIND_REUSE}
# (frames, n_steps, k, interval): timesteps of 8 steps are 49, 43, 36, 30, 24, 18, 12, 5
R = [(100, 8, 2, None), (64, 6, 3, None), (90, 8, 2, (10, 40)), (50, 5, None, None), (70, 7, 1, (0, 30)), (40, 8, 3, (20, 45))]
ARRIVALS = {0: [0, 1], 1: [2], 3: [3, 4], 6: [5]}          # submitted AFTER this many steps


def _acp(T=50):
    betas = torch.linspace(1e-4, 0.02, T, dtype=torch.float64)
    return torch.cumprod(1 - betas, 0).float()


class StubBatch:
    """records what the scheduler asks of the batch"""

    def __init__(self):
        self.regroups, self.steps = [], []

    def regroup(self, plan, args):
        self.regroups.append((len(self.steps) + 1, plan))
        for j, r in enumerate(plan.members):
            r.b, r.row = j, plan.cu[j]

    def step(self, args):
        self.steps.append(args)

    def retire(self, done):
        return [None for _ in done]


def _stream(refresh=True, **kw):
    caps = dict(max_rows=300, max_utterances=3, max_text_rows=4096, guided=True)
    caps.update(kw)
    return GuidedStream(StubBatch(), _acp(), text_dim=TEXT_DIM, hidden_dim=D, refresh=refresh, **caps)


def _submit(s, i, **kw):
    n, steps, k, interval = R[i]
    return s.submit(torch.zeros(8, TEXT_DIM), n, seed=i, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=steps, eta=1.0,
                    guidance_interval=interval, guidance_refresh=k, **kw)


def _want_kinds(i):
    n, steps, k, interval = R[i]
    flags = guided_steps(strided_schedule(_acp().double(), steps, 1.0), interval)
    return [CODE[x] for x in refresh_plan(flags, 1 if k is None else k)[0]]


def _run():
    s = _stream()
    ids, step = {}, 0
    while step == 0 or s.pending or s.active:
        for i in ARRIVALS.get(step, []):
            ids[_submit(s, i).id] = i
        s.step()
        step += 1
    return s, ids


def test_the_requests_cover_every_kind_of_schedule():
    assert [row[0] for row in strided_schedule(_acp().double(), 8, 1.0)] == [49, 43, 36, 30, 24, 18, 12, 5]
    P, F, U = hip.KIND_PLAIN, hip.KIND_REFRESH, hip.KIND_REUSE
    assert _want_kinds(0) == [F, U, F, U, F, U, F, U]
    assert _want_kinds(1) == [F, U, U, F, U, U]
    assert _want_kinds(2) == [P, P, F, U, F, U, F, P]          # the first guided step refreshes; unguided steps are plain
    assert _want_kinds(3) == [F] * 5 and set(_want_kinds(4)) == {P, F}
    assert _want_kinds(5) == [P, F, U, U, F, P, P, P]


def test_every_request_follows_refresh_plan_of_its_own_guided_steps():
    s, ids = _run()
    seen = {i: [] for i in range(len(R))}
    for a in s.batch.steps:
        assert a.in_g == [k == hip.KIND_REFRESH for k in a.kind]
        assert a.G == sum(a.in_g) and a.partner == [sum(a.in_g[:j]) if f else -1 for j, f in enumerate(a.in_g)]
        assert a.S_G == sum(R[ids[h.id]][0] for h, f in zip(a.handles, a.in_g) if f)
        for h, k, per in zip(a.handles, a.kind, a.period):
            seen[ids[h.id]].append(k)
            assert per == (R[ids[h.id]][2] or 1)
    assert seen == {i: _want_kinds(i) for i in range(len(R))}
    # staggered: requests stand at different step indices in one stream step, and every combination of G occurs
    shapes = {(a.B, a.G) for a in s.batch.steps}
    assert any(g == 0 for _, g in shapes) and any(0 < g < b for b, g in shapes) and any(g == b for b, g in shapes), shapes


def test_a_regroup_runs_exactly_when_the_membership_or_the_refresh_set_changes():
    s, ids = _run()
    regrouped = {n for n, _ in s.batch.regroups}
    prev = None
    for n, a in enumerate(s.batch.steps, 1):
        now = ([h.id for h in a.handles], a.in_g)
        assert (n in regrouped) == (now != prev), (n, now, prev)
        prev = now
    assert 1 in regrouped and len(regrouped) < len(s.batch.steps)            # some steps run without one
    for n, plan in s.batch.regroups:
        assert plan.kind == s.batch.steps[n - 1].kind and plan.in_g == s.batch.steps[n - 1].in_g
    # a stream made without refresh hands the batch no kinds
    plain = _stream(refresh=False)
    plain.submit(torch.zeros(8, TEXT_DIM), 64, seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=2)
    plain.step()
    assert plain.batch.regroups[0][1].kind is None and plain.batch.steps[0].kind == [hip.KIND_REFRESH]


@pytest.mark.parametrize("maxB", [1, 3, 4, 32, 33])
@pytest.mark.parametrize("multistep", [False, True])
@pytest.mark.parametrize("infill", [False, True])
def test_step_block_without_refresh_is_unchanged_and_with_refresh_only_appends(maxB, multistep, infill):
    base = step_block_layout(maxB, True, multistep, infill)
    assert base == step_block_layout(maxB, True, multistep, infill, refresh=False) and "kind" not in base
    # the layout as it stood before the argument existed, field by field
    pad = lambda n: (n + 15) // 16 * 16
    f = pad(4 * maxB)
    o_f = pad(16 * maxB) + pad(8 * maxB)
    want = {"t": 0, "seeds": pad(16 * maxB), "f_stride": f}
    for k, name in enumerate(("a", "ce", "cz", "w", "tags", "prompt", "partner", "coef")):
        want[name] = o_f + k * f
    want["phi"] = pad(want["coef"] + (32 * maxB if multistep else 0))
    want["bytes"] = want["phi"] + f
    if infill:
        want["suffix"], want["bytes"] = want["bytes"], want["bytes"] + f
    assert base == want
    ext = step_block_layout(maxB, True, multistep, infill, refresh=True)
    assert ext["kind"] == base["bytes"] and ext["bytes"] == base["bytes"] + f
    assert {k: v for k, v in ext.items() if k not in ("kind", "bytes")} == {k: v for k, v in base.items() if k != "bytes"}


def _request(id_, frames, P=0):
    r = Request(StreamHandle(id_), torch.zeros(8, TEXT_DIM), torch.zeros(5, TEXT_DIM), frames, id_, 2.0, 4, 0.0, None, None,
                prompt=torch.zeros(P, D) if P else None)
    return r


def test_the_regroup_table_carries_the_direction_of_a_survivor_about_to_reuse_only():
    d4 = D // 4
    a, b, c, n = _request(0, 40, P=3), _request(1, 30), _request(2, 20, P=2), _request(3, 10)
    for j, (r, row) in enumerate(((a, 0), (b, 50), (c, 90))):          # where the survivors stand now (holes between them)
        r.b, r.row, r.trow, r.nrow, r.ntm = j, row, 8 * j, 30 + 5 * j, 3 + j
    members = [a, b, c, n]
    kind = [hip.KIND_REUSE, hip.KIND_REFRESH, hip.KIND_PLAIN, hip.KIND_REFRESH]
    plan = Plan(members, [n], True, [k == hip.KIND_REFRESH for k in kind], kind)
    kw = dict(d4=d4, kv16=64, tm16=32, tmod_old16=5000, tmod_new16=6000, new_image={3: (0, 900)}, multistep=False, cu_pad=12)
    segs, _ = regroup_table(plan, **kw)
    carried = [s for s in segs if s[1] == 5 and s[2] == 4]               # the history's slots: source 5, destination 4
    assert carried == [direction_segment(a, plan.cu[0], d4)]
    assert carried[0] == [hip.REGROUP_COPY, 5, 4, 0, (0 + 3) * d4, (0 + 3) * d4, 40 * d4, 0]      # its generated rows, no duplicate
    # moved: the same survivor behind another one
    plan2 = Plan([b, a], [], True, [False, False], [hip.KIND_REUSE, hip.KIND_REUSE])
    segs2, _ = regroup_table(plan2, **{**kw, "new_image": {}})
    assert [s for s in segs2 if s[1] == 5] == [[hip.REGROUP_COPY, 5, 4, 0, 50 * d4, 0, 30 * d4, 0],
                                               [hip.REGROUP_COPY, 5, 4, 0, 3 * d4, (30 + 3) * d4, 40 * d4, 0]]
    # without kinds (a stream made without refresh) the table is the one it was
    plain = Plan(members, [n], True, plan.in_g)
    segs3, _ = regroup_table(plain, **kw)
    assert segs3[:-1] == [s for s in segs if s not in carried][:-1] and len(segs3) == len(segs) - 1
    # the table of a full batch of reusing survivors still fits DeviceBatch's max_seg = 8 maxB + 8
    maxB = 6
    full = [_request(k, 8, P=1) for k in range(maxB)]
    for j, r in enumerate(full):
        r.b, r.row, r.trow, r.nrow, r.ntm = j, 9 * j, 8 * j, 100 + 5 * j, maxB + j
    segs4, _ = regroup_table(Plan(full, [], True, [False] * maxB, [hip.KIND_REUSE] * maxB), **{**kw, "new_image": {}, "cu_pad": 16})
    assert len(segs4) == 6 * maxB + 1 <= 8 * maxB + 8
    assert hip.REGROUP_BUFS == 6


def test_refusals_at_construction_and_submit_leave_the_stream_as_it_was():
    with pytest.raises(NotImplementedError, match="multistep"):
        _stream(solver="dpmpp2m")
    with pytest.raises(NotImplementedError, match="multistep"):
        _stream(infill=True)
    with pytest.raises(ValueError, match="guided"):
        _stream(guided=False)

    class Eng:                                                            # DeviceBatch refuses the same before it makes a buffer
        cfg = None

    for kw, err in ((dict(solver="dpmpp2m"), NotImplementedError), (dict(infill=True), NotImplementedError),
                    (dict(guided=False), ValueError)):
        args = dict(max_rows=64, max_utterances=1, max_text_rows=8, guided=True, refresh=True)
        args.update(kw)
        with pytest.raises(err):
            DeviceBatch(Eng(), **args)
    ok = dict(seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=4)
    text = torch.zeros(8, TEXT_DIM)
    plain = _stream(refresh=False)
    with pytest.raises(ValueError, match="refresh=True"):
        plain.submit(text, 64, guidance_refresh=2, **ok)
    with pytest.raises(ValueError, match="refresh=True"):
        plain.submit(text, 64, guidance_refresh=1, **ok)
    assert plain.pending == 0
    s = _stream()
    for bad in (0, -1, 2.0, True, "2", [2]):
        with pytest.raises(ValueError, match="guidance_refresh"):
            s.submit(text, 64, guidance_refresh=bad, **ok)
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        s.submit(text, 64, guidance_refresh=2, guidance_rescale=0.5, **ok)
    assert s.pending == 0 and s._next_id == 0
    s.submit(text, 64, guidance_refresh=2, guidance_rescale=0.0, **ok)       # phi = 0: no rescale at all
    s.submit(text, 64, guidance_refresh=None, **ok)
    s.submit(text, 64, guidance_refresh=1, guidance_interval=(10, 40), **ok)
    assert s.pending == 3


UPDATE, STEP = "ditto_guided_update_packed_refresh", "ditto_guided_step_packed_refresh_opts"


def test_the_entries_are_declared_exported_and_bound_beside_ditto_hip_h():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ditto_refresh.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ditto_\w+)\s*\(", txt)))
    assert names == sorted([UPDATE, STEP]) == sorted(hip.REFRESH_PROTOTYPES) == sorted(hip.REFRESH_SYMBOLS)
    lib = hip.lib()
    for n in names:
        res, params = hip.REFRESH_PROTOTYPES[n]
        fn = getattr(lib, n)
        assert fn.restype == res == C.c_int and list(fn.argtypes) == [t for _, t in params], n
        assert n not in hip.SYMBOLS
    mixed = [p for p, _ in hip.PROTOTYPES["ditto_guided_step_packed_mixed_opts"][1]]
    step = [p for p, _ in hip.REFRESH_PROTOTYPES[STEP][1]]
    assert sorted(step) == sorted(mixed + ["delta", "kind"])               # the mixed step's arguments plus the two
    upd = [p for p, _ in hip.REFRESH_PROTOTYPES[UPDATE][1]]
    assert sorted(upd) == sorted([p for p, _ in hip.PROTOTYPES["ditto_guided_update_packed_mixed"][1]] + ["delta", "kind"])
    with pytest.raises(TypeError, match="ditto_refresh.h declares no such entry"):
        hip.call("ditto_guided_update_packed_refresh_x")


def _update(**kw):
    p = 4096                                                               # a non-null address: nothing refused here is dereferenced
    args = dict(x2=p, eps2=p, delta=p, noise=None, seeds=None, tags=None, w=p, a=p, ce=p, cz=p, cu=p, partner=p, kind=p, prompt_len=None,
                B=3, G=1, S=40, S_G=20, max_N=20, d=64, stream=None)
    args.update(kw)
    return hip.call(UPDATE, **args)


def test_null_pointers_and_bad_shapes_are_refused_before_any_launch():
    for kw, code, word in ((dict(delta=None), hip.ERR_ARG, "delta"), (dict(kind=None), hip.ERR_ARG, "kind"),
                           (dict(partner=None), hip.ERR_ARG, "partner"), (dict(cu=None), hip.ERR_ARG, "cu"),
                           (dict(seeds=4096), hip.ERR_ARG, "tags"), (dict(x2=None), hip.ERR_ARG, None), (dict(w=None), hip.ERR_ARG, None),
                           (dict(d=96), hip.ERR_SHAPE, None), (dict(B=0), hip.ERR_SHAPE, None), (dict(G=4), hip.ERR_SHAPE, "G"),
                           (dict(S_G=41), hip.ERR_SHAPE, "S_G"), (dict(G=0), hip.ERR_SHAPE, "S_G"), (dict(S_G=0), hip.ERR_SHAPE, "S_G"),
                           (dict(G=3, S_G=2), hip.ERR_SHAPE, "S_G")):
        rc = _update(**kw)
        msg = hip.lib().ditto_last_error().decode()
        assert rc == code, (kw, rc, msg)
        assert UPDATE in msg or word is None, (kw, msg)
        assert word is None or word in msg, (kw, msg)
    # the step: a null model is refused first
    params = [p for p, _ in hip.REFRESH_PROTOTYPES[STEP][1]]
    args = {p: None for p in params}
    args.update(B=1, G=0, S=8, S_G=0, max_N=8, S_T=4, max_T=4, workspace_bytes=0)
    assert hip.call(STEP, **args) == hip.ERR_ARG and STEP in hip.lib().ditto_last_error().decode()
