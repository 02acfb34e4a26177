#!/usr/bin/env python3
"""Continuous batching at C2 (synthetic weights, 32 utterances, the length mix of tools/bench_varlen.py: random.Random(2026), N_b in
[256, 1024], T_b in [64, 1024]; 25 steps, guidance 5.0, eta 1, per-utterance seeds).  ONE process, alternating round by round:
  (a) steady state: GuidedStream.step() with unchanged membership against sample_guided_packed's step (engine.guided_step_packed_)
      on the same 32 utterances — the same forward, so (a) should sit inside the baseline's own round-to-round spread;
  (b) regroup: one departure plus one arrival at that batch — the ditto_regroup_packed launch (µs, effective GB/s over the bytes it
      reads and writes) against the same regroup composed from torch index_select / cat calls (the composition lives HERE, not in the
      product);
  (c) arrival trace: one request every k steps (k = 1: 25 in flight of 32), steps from submission to result (mean, worst) and
      utterance-steps per second, against the best a caller of the closed API can do: sample_guided_packed calls over whatever has
      arrived when the previous call ends (arrivals on the stream's own clock: one per k mean stream steps).
Prints one JSON line and writes it to --out (default profiles/r10_stream_bench.json)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="steps per timed run of (a)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--regroup-reps", type=int, default=20)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--requests", type=int, default=64, help="requests of the arrival trace")
    ap.add_argument("--every", type=int, default=1, help="k: one arrival every k steps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_stream_bench.json"))
    args = ap.parse_args()

    import torch
    from ditto_tts_amd import varlen
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator, strided_schedule
    from ditto_tts_amd.serving import Plan
    from ditto_tts_amd.synth import hash_normal, synthetic_state_dict

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    cfg = PRESETS["C2"]["cfg"]
    B, G, NS = args.batch, 5.0, args.n_steps
    rng = random.Random(2026)
    SL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    d, dt = cfg.hidden_dim, cfg.text_dim
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").eval()
    sg = SpeechGenerator(ditto_model=m, device="cuda")
    eng = m.engine()
    texts = [hash_normal((t, dt), "bench_text", k).cuda() for k, t in enumerate(TL)]
    nulls = [torch.zeros(t, dt, device="cuda") for t in TL]           # (sample_guided_packed expands one null row to the text's rows)
    S, S_T = sum(SL), sum(TL)
    caps = dict(max_rows=S + 1024, max_utterances=B, max_text_rows=2 * S_T + 2048)
    res = {"config": "C2", "B": B, "speech_lengths": SL, "text_lengths": TL, "n_steps": NS, "guidance": G, "eta": 1.0,
           "speech_rows": S, "text_rows": S_T, "steps": args.steps, "rounds": args.rounds}

    with torch.no_grad():
        # ---------------------------------------------------------------- (a) steady state
        stream = sg.guided_stream(guided=True, **caps)
        for k in range(B):
            stream.submit(texts[k], SL[k], seed=1000 + k, guidance=G, null_text_emb=nulls[k], n_steps=cfg.diffusion_steps, eta=1.0)
        stream.step()                                                   # admits all 32

        def rewind():                                                   # (a tool's liberty: keep every utterance far from retiring)
            for r in stream._active:
                r.i = 1

        cu, ct = varlen.cu_from_lengths(SL), varlen.cu_from_lengths(TL)
        tp = torch.cat(texts)
        cond = eng.prepare_text_packed(torch.cat([tp, torch.zeros_like(tp)]), torch.cat([ct, ct[-1] + ct[1:]]))
        offsets = eng.guided_offsets_packed(cu, S, max(SL), True)
        x2 = hash_normal((2 * S, d), "bench_x", 1).cuda()
        x2[S:] = x2[:S]
        t_val, a_, ce_, sg_ = strided_schedule(sg.alphas_cumprod, NS, 1.0)[3]
        coef = [torch.full((B,), v, device="cuda") for v in (a_, ce_, sg_, G)]
        tt = torch.full((2 * B,), t_val, device="cuda", dtype=torch.long)
        seeds = torch.arange(B, device="cuda") + 1000
        base = lambda: eng.guided_step_packed_(x2, cond, tt, B, coef[0], coef[1], coef[2], w=coef[3], seeds=seeds, step=t_val,   # noqa: E731
                                               offsets=offsets)
        runs = {"a_stream_step_ms": [], "baseline_packed_step_ms": []}
        for _ in range(args.rounds):
            rewind()
            runs["a_stream_step_ms"].append(timed(stream.step, args.steps, args.warmup))
            runs["baseline_packed_step_ms"].append(timed(base, args.steps, args.warmup))
        for k, v in runs.items():
            res[k] = statistics.median(v)
            res[k + "_all"] = v
        bl = runs["baseline_packed_step_ms"]
        res["baseline_spread_ms"] = max(bl) - min(bl)
        res["a_minus_baseline_ms"] = res["a_stream_step_ms"] - res["baseline_packed_step_ms"]
        res["a_inside_baseline_spread"] = min(bl) <= res["a_stream_step_ms"] <= max(bl)

        # ---------------------------------------------------------------- (b) regroup: utterance 5 leaves, one arrives
        batch = stream.batch
        rewind()
        members = list(stream._active)
        gone = members[5]
        stream.submit(texts[5], SL[5], seed=5000, guidance=G, null_text_emb=nulls[5], n_steps=NS, eta=1.0)
        new = stream._queue.popleft()
        second = [r for r in members if r is not gone] + [new]
        captured = {}
        run_table = batch._run_table
        batch._run_table = lambda segs, tail, out: (captured.update(segs=segs, tail=tail), run_table(segs, tail, out))[1]
        old_cur, old_B, old_tmod, old_Tt = batch.cur, batch.B, batch._tmod_off, batch.T_text
        batch.regroup(Plan(second, [new], True), stream._step_args(second))
        batch._run_table = run_table
        new_cur, new_tmod = batch.cur, batch._tmod_off
        segs, tail = captured["segs"], captured["tail"]
        moved = sum(16 * s[6] * ((0 if s[0] == 1 else 1) + 1 + (1 if s[7] else 0)) for s in segs)
        batch.cur = old_cur                                             # replay that launch: same sources, same destinations
        us = 1e3 * timed(lambda: run_table(segs, tail, None), args.regroup_reps, 3)
        res["b_regroup_kernel_us"] = us
        res["b_regroup_segments"] = len(segs)
        res["b_regroup_bytes_moved"] = moved
        res["b_regroup_GBps"] = moved / us / 1e3
        res["update_kernel_achievable_GBps"] = 6300.0
        res["b_regroup_fraction_of_update_kernel"] = res["b_regroup_GBps"] / 6300.0
        # the same regroup from torch calls: index_select of the surviving rows + cat with the newcomer's, per buffer
        xo, co, kvb = batch.x[old_cur], batch.cond[old_cur], batch.kv_row
        keep = [r for r in members if r is not gone]
        old_cu, old_ct = [0] + list(torch.tensor(SL).cumsum(0)), [0] + list(torch.tensor(TL).cumsum(0))
        rows = torch.cat([torch.arange(int(old_cu[k]), int(old_cu[k + 1])) for k in range(B) if k != 5]).cuda()
        trows = torch.cat([torch.arange(int(old_ct[k]), int(old_ct[k + 1])) for k in range(B) if k != 5]).cuda()
        nrows = trows + S_T
        slots = torch.tensor([k for k in range(B) if k != 5]).cuda()
        tm = 2 * d * 4
        xT = torch.empty(1, SL[5], d, device="cuda")
        new_img = batch.new_cond
        n_new = new.T * kvb
        new_tm = batch._tmod_offset(new.text_rows)
        S2, ST2 = S, 2 * S_T
        new_seed = torch.tensor([5000], device="cuda")

        def torch_regroup():
            eng.noise_normal_(xT, new_seed, 0xFFFFFFFF)
            half = torch.cat([xo[:S].index_select(0, rows), xT[0]])
            x_new = torch.cat([half, half])
            kv = co[:2 * S_T * kvb].view(-1, kvb)
            kv_new = torch.cat([kv.index_select(0, trows), new_img[:n_new].view(-1, kvb), kv.index_select(0, nrows),
                                new_img[n_new:2 * n_new].view(-1, kvb)])
            tmod = co[old_tmod:old_tmod + 2 * B * tm].view(-1, tm)
            nt = new_img[new_tm:new_tm + 2 * tm].view(-1, tm)
            tm_new = torch.cat([tmod.index_select(0, slots), nt[:1], tmod.index_select(0, slots + B), nt[1:]])
            offs = torch.from_numpy(tail).cuda()
            return x_new, kv_new, tm_new, offs

        tus = 1e3 * timed(torch_regroup, args.regroup_reps, 3)
        x_new, kv_new, tm_new, _ = torch_regroup()
        batch.cur = new_cur
        same = (torch.equal(x_new, batch.x[new_cur][:2 * S2]) and torch.equal(kv_new.view(-1), batch.cond[new_cur][:ST2 * kvb])
                and torch.equal(tm_new.view(-1), batch.cond[new_cur][new_tmod:new_tmod + 2 * B * tm]))
        res["b_torch_composition_us"] = tus
        res["b_torch_over_kernel"] = tus / us
        res["b_torch_composition_same_bits"] = bool(same)
        del stream, batch, x_new, kv_new, tm_new
        torch.cuda.empty_cache()

        # ---------------------------------------------------------------- (c) arrival trace
        Q, k = args.requests, args.every
        stream = sg.guided_stream(guided=True, **caps)
        submitted, finished, steps = {}, {}, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while len(finished) < Q:
            if steps % k == 0 and steps // k < Q:
                q = steps // k
                h = stream.submit(texts[q % B], SL[q % B], seed=q, guidance=G, null_text_emb=nulls[q % B], n_steps=NS, eta=1.0)
                submitted[h.id] = steps
            for h, _ in stream.step():
                finished[h.id] = steps + 1
            steps += 1
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        lat = [finished[i] - submitted[i] for i in submitted]
        step_s = wall / steps
        res.update({"c_requests": Q, "c_every_k_steps": k, "c_stream_steps": steps, "c_stream_wall_s": wall,
                    "c_stream_mean_step_ms": 1e3 * step_s, "c_stream_latency_steps_mean": statistics.mean(lat),
                    "c_stream_latency_steps_worst": max(lat), "c_stream_utterance_steps_per_s": Q * NS / wall})
        # closed calls on the same arrival clock (request q arrives at q * k * step_s seconds)
        arrive = [q * k * step_s for q in range(Q)]
        clock, nxt, lat_c, calls = 0.0, 0, [], 0
        while nxt < Q:
            if arrive[nxt] > clock:
                clock = arrive[nxt]                                      # idle until the next arrival
            batch_q = []
            while nxt < Q and arrive[nxt] <= clock and len(batch_q) < B and sum(SL[q % B] for q in batch_q) + SL[nxt % B] <= caps["max_rows"]:
                batch_q.append(nxt)
                nxt += 1
            ids = [q % B for q in batch_q]
            tq, cq = torch.cat([texts[i] for i in ids]), varlen.cu_from_lengths([TL[i] for i in ids])
            cs = varlen.cu_from_lengths([SL[i] for i in ids])
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            sg.sample_guided_packed(tq, cq, torch.empty(int(cs[-1]), d, device="cuda"), cs, n_steps=NS, eta=1.0, guidance=G,
                                    null_text_emb=torch.zeros(1, dt, device="cuda"), seeds=torch.tensor(batch_q))
            torch.cuda.synchronize()
            clock += time.perf_counter() - c0
            calls += 1
            lat_c += [clock - arrive[q] for q in batch_q]
        res.update({"c_closed_calls": calls, "c_closed_wall_s": clock, "c_closed_latency_steps_mean": statistics.mean(lat_c) / step_s,
                    "c_closed_latency_steps_worst": max(lat_c) / step_s, "c_closed_utterance_steps_per_s": Q * NS / clock,
                    "c_latency_unit": "mean stream step of the trace run (c_stream_mean_step_ms)"})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
