"""Continuous batching on the GPU (ditto_tts_amd/serving.py): the per-utterance-tag update kernel against the scalar-tag kernel called
once per tag, the device regroup against torch indexing, and a request stream through the model — every request, served among
changing neighbours, against sample_guided_packed of that utterance alone: bit for bit under a pinned kernel class, within the batch-
against-solo bound unpinned."""
import ctypes as C

import pytest
import torch

from ditto_tts_amd import hip
from ditto_tts_amd.config import DiTTOConfig
from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.serving import DeviceBatch, GuidedStream, Plan, Request, StreamHandle
from ditto_tts_amd.synth import hash_normal, synthetic_state_dict
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = DiTTOConfig(256, 2, 4, 256, 256, 50)
C2L2 = DiTTOConfig(768, 2, 12, 256, 768, 50)
# the scenario of tests/test_stream_host.py: (frames, text rows, n_steps), per-request guidance and seeds
R = [(160, 48, 4), (64, 20, 6), (97, 33, 8), (200, 7, 4), (130, 40, 5)]
# the bf16-stream class runs the 128-row full-row kernel and refuses launches of fewer than 128 rows; an UNGUIDED solo run of R1 or R2
# is one launch of 64 / 97 rows, so that one case lengthens them (capacities and trace unchanged: 417, 457 and 459 rows in flight)
R_128 = [(160, 48, 4), (128, 20, 6), (129, 33, 8), (200, 7, 4), (130, 40, 5)]
GUIDANCE = [2.0, 3.0, 4.5, 1.0, 5.0]
SEEDS = [101, 202, 303, 404, 505]
T_NULL = 16
ARRIVALS = {0: [0, 1], 2: [2], 3: [3, 4]}          # submitted AFTER this many steps
CAPS = dict(max_rows=512, max_utterances=3, max_text_rows=256)


def _model(cfg, seed=1):
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed))
    return m.to(DEV).eval()


def _texts(cfg, reqs):
    return ([hash_normal((t, cfg.text_dim), "stream_text", k) for k, (_, t, _) in enumerate(reqs)],
            [hash_normal((T_NULL, cfg.text_dim), "stream_null", k) for k in range(len(reqs))])


def _ptr(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- 1. the tag kernel
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("noise", ["philox", "none", "buffer"])
def test_tag_kernel_is_the_scalar_kernel_per_tag(cfg_on, noise):
    lib = hip.lib()
    d, lens = 256, [70, 1, 130, 64, 33]
    B, S = len(lens), sum(lens)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    tags_l = [49, 17, 49, 0xFFFFFFF0, 3]
    rows = 2 * S if cfg_on else S
    x0 = hash_normal((rows, d), "tag_x", 1).to(DEV)
    if cfg_on:
        x0[S:] = x0[:S]
    eps = hash_normal((rows, d), "tag_eps", 2).to(DEV)
    a = torch.tensor([0.9, 1.1, 1.0, 0.7, 1.3], device=DEV)
    ce = torch.tensor([-0.2, 0.3, 0.0, 0.5, -0.1], device=DEV)
    cz = torch.tensor([0.4, 0.0, 0.25, 1.0, 0.0], device=DEV)          # utterances 1 and 4: cz = 0 among noisy ones
    w = torch.tensor([2.0, 3.0, 4.5, 1.0, 5.0], device=DEV) if cfg_on else None
    seeds = torch.tensor([5, -6, 2 ** 40 + 7, 8, 9], dtype=torch.int64, device=DEV) if noise == "philox" else None
    zbuf = hash_normal((S, d), "tag_z", 3).to(DEV) if noise == "buffer" else None
    tags = torch.tensor([t - (1 << 32) if t >= 1 << 31 else t for t in tags_l], dtype=torch.int32, device=DEV)   # uint32 bit patterns
    got = x0.clone()
    hip.check(lib.ditto_guided_update_packed_tags(got.data_ptr(), eps.data_ptr(), _ptr(zbuf), _ptr(seeds), tags.data_ptr(), _ptr(w),
                                                  a.data_ptr(), ce.data_ptr(), cz.data_ptr(), cu.data_ptr(), B, S, max(lens), d,
                                                  int(cfg_on), _s()))
    # the scalar-tag kernel once per distinct tag over the whole batch; utterance b is then read from the run at ITS tag — and, where
    # cz[b] == 0, from the run of the no-noise instantiation
    want = torch.empty_like(x0)
    runs = {}
    for key in sorted(set(tags_l)) + ["nonoise"]:
        y = x0.clone()
        nz = key == "nonoise"
        hip.check(lib.ditto_guided_update_packed(y.data_ptr(), eps.data_ptr(), None if nz else _ptr(zbuf), None if nz else _ptr(seeds),
                                                 0 if nz else key, _ptr(w), a.data_ptr(), ce.data_ptr(), cz.data_ptr(), cu.data_ptr(),
                                                 B, S, max(lens), d, int(cfg_on), _s()))
        runs[key] = y
    for b in range(B):
        lo, hi = int(cu[b]), int(cu[b + 1])
        src = runs["nonoise" if (float(cz[b]) == 0.0 or noise == "none") else tags_l[b]]
        want[lo:hi] = src[lo:hi]
        if cfg_on:
            want[S + lo:S + hi] = src[S + lo:S + hi]
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    if noise == "philox":                       # the tags matter: two utterances at one tag differ from the same two at another
        assert not torch.equal(runs[49][:70], runs[17][:70])


# ---------------------------------------------------------------------------------------------------------------- 2. the regroup
def _req(cfg, k, frames, T, seed, guided, x_T=None):
    text = hash_normal((T, cfg.text_dim), "rg_text", k)
    null = hash_normal((T_NULL + k, cfg.text_dim), "rg_null", k) if guided else None
    return Request(StreamHandle(k), text, null, frames, seed, 2.0 if guided else None, 4, 1.0, x_T, [(49, 1.0, 0.0, 0.0)] * 4)


def _args(stream, members):
    return stream._step_args(members)


@pytest.mark.parametrize("guided", [True, False], ids=["cfg", "nocfg"])
@torch.no_grad()
def test_regroup_matches_torch_indexing(guided):
    cfg = SMALL
    m = _model(cfg)
    eng = m.engine(torch.device("cuda:0"))
    d, halves = cfg.hidden_dim, 2 if guided else 1
    batch = DeviceBatch(eng, max_rows=512, max_utterances=4, max_text_rows=256, guided=guided)
    sched = GuidedStream(batch, torch.linspace(0.99, 0.01, 50), max_rows=512, max_utterances=4, max_text_rows=256, guided=guided,
                         text_dim=cfg.text_dim, hidden_dim=d)
    own = hash_normal((90, d), "rg_xT", 7)
    r0, r1, r2 = _req(cfg, 0, 100, 30, 11, guided), _req(cfg, 1, 90, 9, 12, guided, x_T=own), _req(cfg, 2, 77, 21, 13, guided)
    first = [r0, r1, r2]
    batch.regroup(Plan(first, first, guided), _args(sched, first))
    # what the first batch must hold: x_T drawn per utterance (noise_normal_ packed) or the caller's rows, both halves
    S = 100 + 90 + 77
    x = batch.x[batch.cur]
    for r, lo in ((r0, 0), (r2, 190)):
        xt = torch.empty(1, r.n_frames, d, dtype=torch.float32, device=DEV)
        eng.noise_normal_(xt, torch.tensor([r.seed], device=DEV), 0xFFFFFFFF)
        for h in range(halves):
            assert torch.equal(x[h * S + lo:h * S + lo + r.n_frames], xt[0])
    for h in range(halves):
        assert torch.equal(x[h * S + 100:h * S + 190], own.to(DEV))
    # pretend a step ran: arbitrary state, then r1 leaves and r3 arrives
    x[:halves * S] = hash_normal((halves * S, d), "rg_state", 1).to(DEV)
    old_x, old_cond = x.clone(), batch.cond[batch.cur].clone()
    old_B, old_tmod, old_Tt = batch.B, batch._tmod_off, batch.T_text
    out = batch.retire([r1])
    assert torch.equal(out[0], old_x[100:190])
    nxt = 1 - batch.cur
    batch.x[nxt].fill_(float("nan"))                  # NaN wherever no segment writes, and in the staging buffers' unnamed rows
    batch.cond[nxt].view(torch.int16).fill_(0x7FC0)   # (bf16 NaN; as fp32 pairs NaN too)
    batch.x_T.fill_(float("nan"))
    batch.x[batch.cur][halves * S:] = float("nan")
    r3 = _req(cfg, 3, 120, 40, 14, guided)
    second = [r0, r2, r3]
    plan = Plan(second, [r3], guided)
    batch.regroup(plan, _args(sched, second))
    x, cond = batch.x[batch.cur], batch.cond[batch.cur]
    S2 = 100 + 77 + 120
    xt = torch.empty(1, 120, d, dtype=torch.float32, device=DEV)
    eng.noise_normal_(xt, torch.tensor([14], device=DEV), 0xFFFFFFFF)
    want_x = torch.cat([old_x[0:100], old_x[190:267], xt[0]])
    for h in range(halves):
        assert torch.equal(x[h * S2:(h + 1) * S2], want_x)
    # conditioning: K/V rows and tmod of the survivors from the old image, of the newcomer from its own prepare_text_packed
    kv = batch.kv_row
    ct3 = [0, 40] + ([40 + T_NULL + 3] if guided else [])
    solo = eng.prepare_text_packed(torch.cat([r3.text] + ([r3.null] if guided else [])).to(DEV), ct3).buf
    old_kv = old_cond[:(old_Tt + (sum(r.T_null for r in first) if guided else 0)) * kv].view(-1, kv)
    solo_kv = solo[:r3.text_rows * kv].view(-1, kv)
    text_rows = [old_kv[0:30], old_kv[39:60], solo_kv[0:40]]
    if guided:
        n0 = old_Tt
        text_rows += [old_kv[n0:n0 + T_NULL], old_kv[n0 + 2 * T_NULL + 1:n0 + 3 * T_NULL + 3], solo_kv[40:]]
    want_kv = torch.cat(text_rows)
    S_T2 = want_kv.shape[0]
    assert torch.equal(cond[:S_T2 * kv].view(-1, kv), want_kv)
    tm = 2 * d * 4
    old_tm = old_cond[old_tmod:old_tmod + halves * old_B * tm].view(-1, tm)
    solo_tm = solo[batch._tmod_offset(r3.text_rows):][:halves * tm].view(-1, tm)
    tm_rows = [old_tm[0], old_tm[2], solo_tm[0]] + ([old_tm[old_B], old_tm[old_B + 2], solo_tm[1]] if guided else [])
    got_tm = cond[batch._tmod_off:batch._tmod_off + halves * 3 * tm].view(-1, tm)
    assert torch.equal(got_tm, torch.stack(tm_rows))
    assert torch.isfinite(got_tm.view(torch.float32)).all() and torch.isfinite(want_kv.view(torch.bfloat16).float()).all()
    # offsets: cu (doubled under CFG) and cu_text
    cu = [0, 100, 177, 297]
    cu_t = [0, 30, 51, 91]
    if guided:
        cu = cu + [297 + c for c in cu[1:]]
        cu_t = cu_t + [91 + c for c in (T_NULL, 2 * T_NULL + 2, 3 * T_NULL + 5)]
    offs = batch.offsets.cpu().tolist()
    assert offs[:len(cu)] == cu and offs[batch.cu_pad:batch.cu_pad + len(cu_t)] == cu_t
    assert [(r.b, r.row, r.trow) for r in second] == [(0, 0, 0), (1, 100, 30), (2, 177, 51)]


def test_regroup_clamps_a_bad_table():
    """segments that point outside their buffers write nothing outside them: the guard rows around every buffer stay as they were"""
    lib = hip.lib()
    pool = torch.zeros(3, 64, 4, dtype=torch.float32, device=DEV)          # [guard | buffer | guard], 64 units of 16 bytes each
    pool[0], pool[2] = 7.0, 7.0
    src = torch.arange(32 * 4, dtype=torch.float32, device=DEV).view(32, 4)
    segs = [[0, 0, 0, 0, 0, 60, 32, 0],            # runs past the end of the destination: truncated to 4 units
            [0, 0, 0, 0, 30, 0, 32, 0],            # runs past the end of the source: truncated to 2 units
            [0, 0, 0, 0, 0, 1000, 8, 0],           # destination offset outside: nothing
            [0, 0, 0, 0, 1000, 8, 8, 0],           # source offset outside: nothing
            [0, 5, 0, 0, 0, 16, 8, 0],             # absent source buffer: nothing
            [0, 0, 4, 0, 0, 16, 8, 0],             # absent destination buffer: nothing
            [0, 0, 0, 0, 0, 40, 8, 0xFFFFFFF0],    # dup offset outside: nothing
            [1, 0, 0, 99, 0, 20, 4, 0]]            # seed index outside: clamped to the last seed
    table = torch.tensor([[v - (1 << 32) if v >= 1 << 31 else v for v in sg] for sg in segs], dtype=torch.int32, device=DEV)
    seeds = torch.tensor([3, 4], dtype=torch.int64, device=DEV)
    n = hip.REGROUP_BUFS
    sp, sb, dp, db = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
    sp[0], sb[0] = src.data_ptr(), src.numel() * 4
    dp[0], db[0] = pool[1].data_ptr(), 64 * 16
    hip.check(lib.ditto_regroup_packed(table.data_ptr(), len(segs), sp, sb, dp, db, n, seeds.data_ptr(), 2, 32 * 16, _s()))
    got = pool.cpu()
    assert torch.equal(got[0], torch.full((64, 4), 7.0)) and torch.equal(got[2], torch.full((64, 4), 7.0))
    assert torch.equal(got[1, 60:64], src[0:4].cpu()) and torch.equal(got[1, 0:2], src[30:32].cpu())
    z = torch.empty(1, 16, dtype=torch.float32, device=DEV)
    hip.check(lib.ditto_noise_normal(z.data_ptr(), seeds[1:].data_ptr(), 0xFFFFFFFF, 1, 16, _s()))
    assert torch.equal(got[1, 20:24].reshape(-1), z.cpu().reshape(-1))
    untouched = torch.ones(64, dtype=torch.bool)
    untouched[60:64] = untouched[0:2] = untouched[20:24] = False
    assert torch.equal(got[1][untouched], torch.zeros(int(untouched.sum()), 4))


# ---------------------------------------------------------------------------------------------------------------- 3-6. the stream
def _run_stream(sg, cfg, reqs, guided, order=None, arrivals=ARRIVALS, n_steps=None, class_rows=None):
    texts, nulls = _texts(cfg, reqs)
    stream = sg.guided_stream(guided=guided, class_rows=class_rows, **CAPS)
    handles, results, in_flight = {}, {}, []
    step = 0
    while step == 0 or stream.pending or stream.active:
        ks = arrivals.get(step, [])
        for k in (ks if order is None else [order[i] for i in ks]):
            kw = dict(guidance=GUIDANCE[k], null_text_emb=nulls[k]) if guided else {}
            handles[stream.submit(texts[k], reqs[k][0], seed=SEEDS[k], n_steps=n_steps or reqs[k][2], eta=1.0, **kw).id] = k
        done = stream.step()
        step += 1
        in_flight.append(stream.active)
        for h, out in done:
            results[handles[h.id]] = out.clone()
    return results, step


def _solo(sg, cfg, reqs, k, guided, n_steps=None):
    texts, nulls = _texts(cfg, reqs)
    n, t, steps = reqs[k]
    kw = dict(guidance=GUIDANCE[k], null_text_emb=nulls[k].to(DEV), null_text_cu_seqlens=[0, T_NULL]) if guided else {}
    return sg.sample_guided_packed(texts[k].to(DEV), [0, t], torch.zeros(n, cfg.hidden_dim, device=DEV), [0, n], n_steps=n_steps or steps,
                                   eta=1.0, seeds=torch.tensor([SEEDS[k]]), **kw)


@pytest.mark.parametrize("guided", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("cfg,rows", [(SMALL, 4096), (C2L2, 17408)], ids=["fp32_stream", "bf16_stream"])
@torch.no_grad()
def test_stream_equals_solo_runs_bit_for_bit_under_the_pin(cfg, rows, guided):
    reqs = R_128 if (cfg is C2L2 and not guided) else R
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    with hip.batch_class(rows):
        if cfg is C2L2:
            assert hip.stream_is_bf16(cfg, 1, 128)
        got, steps = _run_stream(sg, cfg, reqs, guided)
        assert steps == 11 and sorted(got) == [0, 1, 2, 3, 4]
        for k in range(5):
            solo = _solo(sg, cfg, reqs, k, guided)
            assert got[k].shape == solo.shape == (reqs[k][0], cfg.hidden_dim)
            assert torch.isfinite(solo).all()
            assert torch.equal(got[k], solo), f"request {k}: rel-L2 {rel_l2(got[k].cpu(), solo.cpu()):.3e} against its solo run"


@torch.no_grad()
def test_class_rows_argument_pins_like_the_scope():
    cfg = SMALL
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    got, _ = _run_stream(sg, cfg, R, True, class_rows=4096)
    with hip.batch_class(4096):
        for k in range(5):
            assert torch.equal(got[k], _solo(sg, cfg, R, k, True))


@pytest.mark.parametrize("guided", [True, False], ids=["cfg", "nocfg"])
@torch.no_grad()
def test_stream_unpinned_within_the_batch_against_solo_bound(guided):
    cfg = SMALL
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    got, steps = _run_stream(sg, cfg, R, guided)
    assert steps == 11
    for k in range(5):
        r = rel_l2(got[k].cpu(), _solo(sg, cfg, R, k, guided).cpu())
        print(f"request {k}: rel-L2 {r:.3e} against its solo run (unpinned)")
        assert r <= 2e-2, f"request {k}: rel-L2 {r:.3e} against its solo run"


@torch.no_grad()
def test_order_of_submission_changes_no_bit():
    cfg = SMALL
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    with hip.batch_class(4096):
        a, _ = _run_stream(sg, cfg, R, True)
        b, _ = _run_stream(sg, cfg, R, True, order=[3, 2, 4, 0, 1])
    for k in range(5):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("guided", [True, False], ids=["cfg", "nocfg"])
@torch.no_grad()
def test_same_schedule_stream_equals_one_closed_call(guided):
    cfg = SMALL
    reqs = R[:3]
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    texts, nulls = _texts(cfg, reqs)
    cu = [0, 160, 224, 321]
    ct = [0, 48, 68, 101]
    with hip.batch_class(4096):
        got, steps = _run_stream(sg, cfg, reqs, guided, arrivals={0: [0, 1, 2]}, n_steps=6)
        assert steps == 6
        kw = dict(guidance=GUIDANCE[:3], null_text_emb=torch.cat(nulls).to(DEV),
                  null_text_cu_seqlens=[0, T_NULL, 2 * T_NULL, 3 * T_NULL]) if guided else {}
        closed = sg.sample_guided_packed(torch.cat(texts).to(DEV), ct, torch.zeros(321, cfg.hidden_dim, device=DEV), cu, n_steps=6,
                                         eta=1.0, seeds=torch.tensor(SEEDS[:3]), **kw)
    for k in range(3):
        assert torch.equal(got[k], closed[cu[k]:cu[k + 1]]), k


@torch.no_grad()
def test_caller_x_T_and_steady_state_allocations():
    """a request that brings its own x_T equals the solo run started from it (cond_by_audio); steady-state steps allocate nothing"""
    cfg = SMALL
    sg = SpeechGenerator(ditto_model=_model(cfg, seed=3), device=DEV)
    texts, nulls = _texts(cfg, R)
    xT = hash_normal((160, cfg.hidden_dim), "own_xT", 1)
    with hip.batch_class(4096):
        stream = sg.guided_stream(guided=True, **CAPS)
        stream.submit(texts[0], 160, seed=SEEDS[0], guidance=2.0, null_text_emb=nulls[0], n_steps=8, eta=1.0, x_T=xT)
        assert stream.step() == [] and stream.step() == []
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        for _ in range(4):
            assert stream.step() == []
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
        (h, out), = stream.drain()
        solo = sg.sample_guided_packed(texts[0].to(DEV), [0, 48], xT.to(DEV), [0, 160], n_steps=8, eta=1.0, guidance=2.0,
                                       null_text_emb=nulls[0].to(DEV), null_text_cu_seqlens=[0, T_NULL], seeds=torch.tensor([SEEDS[0]]),
                                       cond_by_audio=True)
    assert torch.equal(out, solo)
