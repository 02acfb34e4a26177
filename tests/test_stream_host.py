"""The scheduler of a request stream (ditto_tts_amd/serving.py GuidedStream) against a stub batch that records calls: FIFO admission
under three capacities, per-utterance schedules, contiguous offsets, retirement, refusals and submit validation.  No GPU."""
import pytest
import torch

from ditto_tts_amd.sampler import strided_schedule
from ditto_tts_amd.serving import GuidedStream

TEXT_DIM, D = 32, 64
# (frames, text rows, n_steps)
R = [(160, 48, 4), (64, 20, 6), (97, 33, 8), (200, 7, 4), (130, 40, 5)]
GUIDANCE = [2.0, 3.0, 4.5, 1.0, 5.0]


def _acp(T=50):
    betas = torch.linspace(1e-4, 0.02, T, dtype=torch.float64)
    return torch.cumprod(1 - betas, 0).float()


class StubBatch:
    """records what the scheduler asks of the batch"""

    def __init__(self):
        self.regroups, self.steps, self.retired = [], [], []

    def regroup(self, plan, args):
        self.regroups.append((len(self.steps) + 1, [r.handle.id for r in plan.members], [r.handle.id for r in plan.newcomers],
                              list(plan.cu), list(plan.cu_text), None if plan.cu_null is None else list(plan.cu_null)))
        for j, r in enumerate(plan.members):       # what DeviceBatch.regroup leaves on a request
            r.b, r.row = j, plan.cu[j]

    def step(self, args):
        self.steps.append(args)

    def retire(self, done):
        self.retired.append((len(self.steps), [r.handle.id for r in done]))
        return [("latents", r.handle.id) for r in done]


def _stream(guided=True, **kw):
    caps = dict(max_rows=512, max_utterances=3, max_text_rows=4096)
    caps.update(kw)
    return GuidedStream(StubBatch(), _acp(), guided=guided, text_dim=TEXT_DIM, hidden_dim=D, **caps)


def _submit(s, k, eta=1.0, guided=True):
    n, t, steps = R[k]
    kw = dict(guidance=GUIDANCE[k], null_text_emb=torch.zeros(5, TEXT_DIM)) if guided else {}
    return s.submit(torch.zeros(t, TEXT_DIM), n, seed=100 + k, n_steps=steps, eta=eta, **kw)


@pytest.mark.parametrize("guided", [True, False])
def test_scenario_trace(guided):
    s = _stream(guided)
    h = {}
    arrivals = {0: [0, 1], 2: [2], 3: [3, 4]}          # submitted AFTER this many steps
    results, in_flight = {}, []
    step = 0
    while step == 0 or s.pending or s.active:
        for k in arrivals.get(step, []):
            h[k] = _submit(s, k, guided=guided)
        done = s.step()
        step += 1
        in_flight.append(list(s.batch.steps[-1].handles))
        for handle, out in done:
            results[handle.id] = (step, out)
    assert step == 11 and len(s.batch.steps) == 11
    ids = lambda hs: [x.id for x in hs]
    want = {1: [0, 1], 2: [0, 1], 3: [0, 1, 2], 4: [0, 1, 2], 5: [1, 2, 3], 6: [1, 2, 3], 7: [2, 3, 4], 8: [2, 3, 4], 9: [2, 4],
            10: [2, 4], 11: [4]}
    for k, members in want.items():
        assert ids(in_flight[k - 1]) == members, k
    rows = {k: s.batch.steps[k - 1].S for k in want}
    assert (rows[3], rows[5], rows[7]) == (321, 361, 427)
    assert {i: r[0] for i, r in results.items()} == {0: 4, 1: 6, 3: 8, 2: 10, 4: 11}
    assert all(out == ("latents", i) for i, (_, out) in results.items())
    assert s.batch.retired == [(4, [0]), (6, [1]), (8, [3]), (10, [2]), (11, [4])]
    # R4 (submitted with R3 after step 3) waits behind it: first in flight at step 7, R3 at step 5
    first = {i: min(k for k in want if i in want[k]) for i in range(5)}
    assert first == {0: 1, 1: 1, 2: 3, 3: 5, 4: 7}
    # membership changed at steps 1, 3, 5, 7, 9, 11: a regroup each, offsets contiguous from 0
    assert [g[0] for g in s.batch.regroups] == [1, 3, 5, 7, 9, 11]
    for _, members, newcomers, cu, cu_text, cu_null in s.batch.regroups:
        assert cu[0] == 0 and cu_text[0] == 0
        assert [b - a for a, b in zip(cu, cu[1:])] == [R[i][0] for i in members]
        assert [b - a for a, b in zip(cu_text, cu_text[1:])] == [R[i][1] for i in members]
        assert (cu_null == [5 * j for j in range(len(members) + 1)]) if guided else cu_null is None
        assert set(newcomers) <= set(members)
    assert [g[2] for g in s.batch.regroups] == [[0, 1], [2], [3], [4], [], []]


def test_every_utterance_follows_its_own_schedule():
    s = _stream(True)
    arrivals = {0: [0, 1], 2: [2], 3: [3, 4]}
    step = 0
    while step == 0 or s.pending or s.active:
        for k in arrivals.get(step, []):
            _submit(s, k, eta=1.0 if k % 2 == 0 else 0.0)
        s.step()
        step += 1
    acp = _acp()
    index = {i: 0 for i in range(5)}
    for a in s.batch.steps:
        assert a.B == len(a.handles) and a.S == sum(R[x.id][0] for x in a.handles)
        assert a.max_N == max(R[x.id][0] for x in a.handles)
        assert a.S_T == sum(R[x.id][1] + 5 for x in a.handles) and a.max_T == max(R[x.id][1] for x in a.handles)
        for j, x in enumerate(a.handles):
            i = x.id
            sched = strided_schedule(acp, R[i][2], 1.0 if i % 2 == 0 else 0.0)
            t, ca, ce, sigma = sched[index[i]]
            assert (a.t[j], a.a[j], a.ce[j], a.cz[j], a.tags[j]) == (t, ca, ce, sigma, t)
            assert a.w[j] == GUIDANCE[i] and a.seeds[j] == 100 + i
            index[i] += 1
    assert index == {i: R[i][2] for i in range(5)}
    assert len(s._schedules) == 5               # cached per (n_steps, eta)


def test_schedules_are_cached_per_steps_and_eta():
    s = _stream(False)
    for _ in range(3):
        s.submit(torch.zeros(4, TEXT_DIM), 64, seed=1, n_steps=5, eta=0.5)
    s.submit(torch.zeros(4, TEXT_DIM), 64, seed=1, n_steps=5, eta=0.0)
    assert sorted(s._schedules) == [(5, 0.0), (5, 0.5)]


def test_fifo_stops_at_the_first_request_that_does_not_fit():
    s = _stream(False, max_rows=300, max_utterances=8)
    s.submit(torch.zeros(4, TEXT_DIM), 200, seed=1, n_steps=2)
    s.submit(torch.zeros(4, TEXT_DIM), 150, seed=2, n_steps=2)      # does not fit beside the first
    s.submit(torch.zeros(4, TEXT_DIM), 50, seed=3, n_steps=2)       # would fit, but may not overtake
    s.step()
    assert [x.id for x in s.batch.steps[-1].handles] == [0] and s.pending == 2 and s.active == 1
    out = s.drain()
    assert [h.id for h, _ in out] == [0, 1, 2]
    assert [[x.id for x in a.handles] for a in s.batch.steps] == [[0], [0], [1, 2], [1, 2]]
    assert s.step() == [] and len(s.batch.steps) == 4                # nothing in flight: nothing launched


def test_text_row_capacity_counts_null_rows():
    s = _stream(True, max_text_rows=60)
    kw = dict(guidance=1.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=1)
    s.submit(torch.zeros(30, TEXT_DIM), 64, seed=1, **kw)           # 35 conditioning rows
    s.submit(torch.zeros(25, TEXT_DIM), 64, seed=2, **kw)           # 30 more: 65 > 60
    s.step()
    assert [x.id for x in s.batch.steps[-1].handles] == [0]
    with pytest.raises(ValueError, match="max_text_rows"):
        s.submit(torch.zeros(56, TEXT_DIM), 64, seed=3, **kw)        # 61 rows can never fit


def test_submit_validation_and_refusals():
    s = _stream(True)
    ok = dict(seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM), n_steps=4)
    text = torch.zeros(8, TEXT_DIM)
    bad = [
        (dict(text_emb=torch.zeros(8, TEXT_DIM + 1)), {}),                         # wrong text_dim
        (dict(text_emb=torch.zeros(0, TEXT_DIM)), {}),                             # empty text
        (dict(text_emb=torch.zeros(8, TEXT_DIM, dtype=torch.long)), {}),
        (dict(text_emb=[[0.0] * TEXT_DIM]), {}),
        (dict(n_frames=0), {}), (dict(n_frames=64.0), {}), (dict(n_frames=True), {}),
        (dict(n_frames=513), {}),                                                  # can never fit max_rows
        ({}, dict(n_steps=0)), ({}, dict(n_steps=51)), ({}, dict(n_steps=2.5)),
        ({}, dict(eta=-1.0)), ({}, dict(eta=float("nan"))), ({}, dict(eta="1")),
        ({}, dict(guidance=None)), ({}, dict(guidance=float("inf"))), ({}, dict(guidance=True)),
        ({}, dict(null_text_emb=None)), ({}, dict(null_text_emb=torch.zeros(5, TEXT_DIM - 1))),
        ({}, dict(seed=1.5)), ({}, dict(seed=2 ** 63)),
        ({}, dict(x_T=torch.zeros(63, D))), ({}, dict(x_T=torch.zeros(64, D, dtype=torch.long))),
    ]
    for pos, kw in bad:
        args = dict(text_emb=text, n_frames=64)
        args.update(pos)
        with pytest.raises(ValueError):
            s.submit(args["text_emb"], args["n_frames"], **{**ok, **kw})
    assert s.pending == 0                                                          # a refused request leaves no trace
    h = s.submit(text, 64, x_T=torch.zeros(64, D), **ok)
    assert s.pending == 1 and h.id == 0
    # an unguided stream refuses guided requests (and the other way round, above)
    u = _stream(False)
    with pytest.raises(ValueError, match="unguided"):
        u.submit(text, 64, seed=1, guidance=2.0, null_text_emb=torch.zeros(5, TEXT_DIM))
    with pytest.raises(ValueError, match="unguided"):
        u.submit(text, 64, seed=1, guidance=2.0)
    u.submit(text, 64)                                                             # seed=None: drawn from torch's generator
    assert u.pending == 1
    for cap in ("max_rows", "max_utterances", "max_text_rows"):
        with pytest.raises(ValueError, match=cap):
            _stream(True, **{cap: 0})


def test_seedless_requests_draw_reproducible_seeds():
    seeds = []
    for _ in range(2):
        torch.manual_seed(7)
        s = _stream(False)
        s.submit(torch.zeros(4, TEXT_DIM), 64, n_steps=1)
        s.submit(torch.zeros(4, TEXT_DIM), 64, n_steps=1)
        s.step()
        seeds.append(list(s.batch.steps[-1].seeds))
    assert seeds[0] == seeds[1] and seeds[0][0] != seeds[0][1]


def test_refusals_of_models_without_the_fused_attention():
    """head_dim != 64 and fp8 linears are refused through require_fused_attention before any buffer is made"""
    from ditto_tts_amd.config import DiTTOConfig
    from ditto_tts_amd.serving import DeviceBatch

    class Eng:
        def __init__(self, cfg):
            self.cfg = cfg

    with pytest.raises(NotImplementedError, match="head_dim 64"):
        DeviceBatch(Eng(DiTTOConfig(256, 2, 2, 256, 256, 50)), max_rows=64, max_utterances=1, max_text_rows=8, guided=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        DeviceBatch(Eng(DiTTOConfig(256, 2, 4, 256, 256, 50, fp8_linear=True)), max_rows=64, max_utterances=1, max_text_rows=8,
                    guided=True)
