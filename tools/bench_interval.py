#!/usr/bin/env python3
"""Guidance in a limited interval at C2 (synthetic weights, B = 32, the lengths of tools/bench_varlen.py: random.Random(2026), N_b in
[256, 1024], T_b in [64, 1024]; 25 steps, guidance 5.0, eta 1, seeds), in ONE process, alternating round by round:
  (a) sample_guided_packed with no interval against the same call on the PARENT commit's library (--parent-lib: a second
      libditto_hip.so loaded beside this tree's): the same launch sequence, so (a) should sit inside the baseline's own
      round-to-round spread.  ONE model is alive at a time: every timed call builds its generator (weights, arena, workspace) from
      a freed device, so both libraries meet the same memory placement, and the order of the three arms — this tree, the parent,
      the parent AGAIN (the A/A pair: what two instances of one library differ by) — rotates round by round;
  (b) the closed call with an interval over the middle 13 of the 25 steps: ms per call, against 13 guided + 12 unguided steps at
      their existing per-step costs (the calls with every step guided and with no guidance, / 25) — the difference is reported;
  (c) the arrival trace of tools/bench_stream.py (one request per step), every request with that interval, against the same trace
      without intervals: utterance-steps per second, mean and worst steps to completion, the number of regroups, and the cost of a
      regroup that only a change of the guided set caused (none occurs in that trace: every step has an arrival or a retirement);
  (d) the regroup caused by a change of the guided set ALONE: all 32 requests admitted at step 0, every second one with that
      interval, no arrivals — the guided set goes half -> everyone -> half at the interval's edges, and those two steps regroup
      with unchanged members.  ms per such regroup (events around the call: conditioning copies, uploads, the one launch), beside
      the arrival regroups of (c), the first regroup (32 newcomers) and the mixed / all-guided steps of the same run;
  the mixed update alone (ditto_guided_update_packed_mixed, half the utterances guided, Philox noise): µs and TB/s over 20 B per
  guided and 12 B per unguided element, beside the all-guided and unguided per-utterance-tag kernels on the same batch.
Prints one JSON line and writes it to --out (default profiles/r18_interval_bench.json)."""
import argparse
import gc
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="libditto_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_interval_bench.json"))
    args = ap.parse_args()

    import ctypes as C

    import torch
    from ditto_tts_amd import hip
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator, guided_steps, strided_schedule
    from ditto_tts_amd.synth import cosine_betas, hash_normal, synthetic_state_dict

    def timed(fn, steps=1, warmup=1):
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

    def rounds(pairs, steps=1, warmup=1):
        runs = {k: [] for k, _ in pairs}
        for _ in range(args.rounds):
            for k, fn in pairs:
                runs[k].append(timed(fn, steps, warmup))
        out = {}
        for k, v in runs.items():
            out[k] = statistics.median(v)
            out[k + "_all"] = v
        return out

    def cumulate(lens):
        out = [0]
        for n in lens:
            out.append(out[-1] + n)
        return out

    cfg = PRESETS["C2"]["cfg"]
    B, d, NS, W = args.batch, cfg.hidden_dim, args.n_steps, 5.0
    rng = random.Random(2026)
    NL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    cu, ct = cumulate(NL), cumulate(TL)
    S = cu[-1]

    state = synthetic_state_dict(cfg, seed=1)
    new_lib = hip.lib()

    def generator(lib=None):
        """a generator whose engine is bound to `lib` (default: this tree's library) for its lifetime"""
        hip._lib = lib or new_lib
        try:
            m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
            m.load_state_dict(state)
            g = SpeechGenerator(ditto_model=m.to("cuda").eval(), device="cuda")
            assert g.ditto_model.engine(torch.device("cuda:0")).lib is (lib or new_lib)
        finally:
            hip._lib = new_lib
        return g

    audio = hash_normal((S, d), "bench_interval_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_interval_text", 2).cuda()
    seeds = torch.arange(B, device="cuda") + 1000
    null = torch.zeros(1, cfg.text_dim, device="cuda")
    res = {"config": "C2", "B": B, "lengths": NL, "text_lengths": TL, "rows": S, "rounds": args.rounds, "n_steps": NS, "guidance": W}
    with torch.no_grad():
        table = torch.cumprod(1 - cosine_betas(cfg.diffusion_steps), 0)          # (the timesteps depend on the table's length only)
        taus = [row[0] for row in strided_schedule(table, NS, 1.0)]
        first = (NS - 13) // 2
        interval = (taus[first + 12], taus[first])
        assert sum(guided_steps([(t,) for t in taus], interval)) == 13
        res["interval"], res["guided_steps"] = list(interval), 13

        def call(g, **kw):
            gkw = dict(guidance=W, null_text_emb=null) if kw.pop("guided", True) else {}
            return lambda: g.sample_guided_packed(text, ct, audio, cu, n_steps=NS, eta=1.0, seeds=seeds, **gkw, **kw)

        # ---------------------------------------------------------------- (a) no interval, against the parent library
        arms = [("a_no_interval_ms", None)]
        if args.parent_lib:
            old = C.CDLL(os.path.abspath(args.parent_lib))
            for name, (r, a) in hip.SYMBOLS.items():
                if hasattr(old, name):
                    getattr(old, name).restype, getattr(old, name).argtypes = r, a
            assert old.ditto_abi_version() == new_lib.ditto_abi_version() and not hasattr(old, "ditto_guided_step_packed_mixed_opts")
            arms += [("a_parent_ms", old), ("a_parent_again_ms", old)]
        runs, outputs = {k: [] for k, _ in arms}, {}
        for rnd in range(args.rounds):
            for k, lib in arms[rnd % len(arms):] + arms[:rnd % len(arms)]:
                g = generator(lib)
                f = call(g)
                runs[k].append(timed(f))
                if rnd == 0:
                    outputs[k] = f().cpu()
                del g, f
                gc.collect()
                torch.cuda.empty_cache()
        for k, v in runs.items():
            res[k], res[k + "_all"] = statistics.median(v), v
        if args.parent_lib:
            assert torch.equal(outputs["a_no_interval_ms"], outputs["a_parent_ms"])
            p_all = res["a_parent_ms_all"]
            res["a_ratio_over_parent"] = res["a_no_interval_ms"] / res["a_parent_ms"]
            res["a_parent_again_ratio_over_parent"] = res["a_parent_again_ms"] / res["a_parent_ms"]
            res["a_parent_rounds_max_over_min"] = max(p_all) / min(p_all)
            res["a_inside_parent_spread"] = min(p_all) <= res["a_no_interval_ms"] <= max(p_all)
        sg = generator()
        # ---------------------------------------------------------------- (b) the middle 13 of 25 steps
        res.update(rounds([("b_interval_ms", call(sg, guidance_interval=interval)), ("b_every_step_guided_ms", call(sg)),
                           ("b_unguided_ms", call(sg, guided=False))]))
        res["b_guided_step_ms"], res["b_unguided_step_ms"] = res["b_every_step_guided_ms"] / NS, res["b_unguided_ms"] / NS
        res["b_expected_ms"] = 13 * res["b_guided_step_ms"] + (NS - 13) * res["b_unguided_step_ms"]
        res["b_difference_ms"] = res["b_interval_ms"] - res["b_expected_ms"]
        res["b_ratio_over_every_step_guided"] = res["b_interval_ms"] / res["b_every_step_guided_ms"]

        # ---------------------------------------------------------------- (c) the arrival trace
        texts = [text[ct[k]:ct[k + 1]].contiguous() for k in range(B)]
        nulls = [torch.zeros(t, cfg.text_dim, device="cuda") for t in TL]
        caps = dict(max_rows=S + 1024, max_utterances=B, max_text_rows=2 * ct[-1] + 2048)

        def instrument(stream):
            """time every regroup and every step of `stream` with events; kinds: a regroup "g" (the guided set alone changed),
            "m" (members changed); a step by its number of guided utterances"""
            regroup, step, log = stream.batch.regroup, stream.batch.step, {"regroup": [], "step": []}

            def pair():
                return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed_regroup(plan, a):
                kind = "g" if not plan.newcomers and not stream._dirty else "m"
                e = pair()
                e[0].record()
                regroup(plan, a)
                e[1].record()
                log["regroup"].append((kind, len(plan.newcomers), e))

            def timed_step(a):
                e = pair()
                e[0].record()
                step(a)
                e[1].record()
                log["step"].append((a.G, a.B, e))

            stream.batch.regroup, stream.batch.step = timed_regroup, timed_step
            return log

        def ms(events):
            return [a.elapsed_time(b) for a, b in events]

        def trace(iv):
            stream = sg.guided_stream(guided=True, **caps)
            log = instrument(stream)
            Q, submitted, finished, steps = args.requests, {}, {}, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while len(finished) < Q:
                if steps < Q:
                    h = stream.submit(texts[steps % B], NL[steps % B], seed=steps, guidance=W, null_text_emb=nulls[steps % B], n_steps=NS,
                                      eta=1.0, guidance_interval=iv)
                    submitted[h.id] = steps
                for h, _ in stream.step():
                    finished[h.id] = steps + 1
                steps += 1
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            lat = [finished[i] - submitted[i] for i in submitted]
            only = ms([e for k, _, e in log["regroup"] if k == "g"])
            full = ms([e for k, n, e in log["regroup"] if k == "m" and n == 1])
            return {"stream_steps": steps, "wall_s": wall, "utterance_steps_per_s": Q * NS / wall, "latency_steps_mean": statistics.mean(lat),
                    "latency_steps_worst": max(lat), "regroups": len(log["regroup"]), "regroups_by_guided_set_alone": len(only),
                    "arrival_regroup_ms_median": statistics.median(full) if full else None}

        def edges():
            """(d): ms of the regroups the guided set alone caused, and of the steps around them"""
            stream = sg.guided_stream(guided=True, **caps)
            log = instrument(stream)
            for k in range(B):
                stream.submit(texts[k], NL[k], seed=k, guidance=W, null_text_emb=nulls[k], n_steps=NS, eta=1.0,
                              guidance_interval=interval if k % 2 else None)
            while stream.pending or stream.active:
                stream.step()
            torch.cuda.synchronize()
            assert [(k, n) for k, n, _ in log["regroup"]] == [("m", B), ("g", 0), ("g", 0)], [(k, n) for k, n, _ in log["regroup"]]
            assert sorted({g for g, _, _ in log["step"]}) == [B // 2, B]
            return {"first_regroup_ms": ms([log["regroup"][0][2]])[0], "g_regroup_ms": ms([e for k, _, e in log["regroup"] if k == "g"]),
                    "mixed_step_ms": ms([e for g, _, e in log["step"] if g == B // 2]),
                    "all_guided_step_ms": ms([e for g, _, e in log["step"] if g == B])}

        trace(interval)                                                          # warm-up: workspaces, allocator
        runs = {"c_interval": [], "c_no_interval": []}
        for _ in range(args.rounds):
            runs["c_interval"].append(trace(interval))
            runs["c_no_interval"].append(trace(None))
        for k, v in runs.items():
            res[k] = sorted(v, key=lambda r: r["wall_s"])[len(v) // 2]
            res[k + "_wall_s_all"] = [r["wall_s"] for r in v]
        res["c_requests"] = args.requests
        res["c_throughput_ratio"] = res["c_interval"]["utterance_steps_per_s"] / res["c_no_interval"]["utterance_steps_per_s"]
        # ---------------------------------------------------------------- (d) the regroup a change of the guided set alone causes
        edges()
        runs = [edges() for _ in range(args.rounds)]
        g_all = [v for r in runs for v in r["g_regroup_ms"]]
        row, off = C.c_size_t(0), C.c_size_t(0)
        hip.check(hip.lib().ditto_regroup_cond_layout(C.byref(sg.ditto_model.engine(torch.device("cuda:0"))._ccfg), 1, C.byref(row),
                                                      C.byref(off)))
        # what one such regroup writes into the other buffer pair: the state rows (about 1.5 S: half or all of the copies), every K/V
        # row of the image (text and null), tmod
        moved = S * d * 4 * 1.5 + (2 * ct[-1]) * row.value + 2 * B * 2 * d * 4
        res["d_guided_set_regroup_ms_median"] = statistics.median(g_all)
        res["d_guided_set_regroup_ms_all"] = g_all
        res["d_guided_set_regroup_bytes_written_approx"] = moved
        res["d_guided_set_regroup_effective_TBps_read_plus_write"] = 2 * moved / (statistics.median(g_all) * 1e-3) / 1e12
        res["d_first_regroup_32_newcomers_ms_median"] = statistics.median(r["first_regroup_ms"] for r in runs)
        res["d_mixed_step_ms_median"] = statistics.median(v for r in runs for v in r["mixed_step_ms"])
        res["d_all_guided_step_ms_median"] = statistics.median(v for r in runs for v in r["all_guided_step_ms"])
        res["d_regroup_over_all_guided_step"] = res["d_guided_set_regroup_ms_median"] / res["d_all_guided_step_ms_median"]
        torch.cuda.empty_cache()

        # ---------------------------------------------------------------- the mixed update alone
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        guided = [b for b in range(B) if b % 2 == 0]
        cu_g = cumulate([NL[b] for b in guided])
        S_G = cu_g[-1]
        x2 = torch.cat([audio, audio])
        eps2 = hash_normal((2 * S, d), "bench_interval_eps2", 5).cuda()
        a, ce, cz, w = (torch.full((B,), v, device="cuda") for v in (0.98, -0.05, 0.1, W))
        tags = torch.full((B,), 49, dtype=torch.int32, device="cuda")
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
        off_mixed, off_all = i32(cu + [S + c for c in cu_g[1:]]), i32(cu + [S + c for c in cu[1:]])
        partner = i32([guided.index(b) if b in guided else -1 for b in range(B)])
        head = (x2.data_ptr(), eps2.data_ptr(), None, seeds.data_ptr(), tags.data_ptr(), w.data_ptr(), a.data_ptr(), ce.data_ptr(),
                cz.data_ptr())
        ks = (("update_mixed_ms", lambda: hip.check(lib.ditto_guided_update_packed_mixed(
                  *head, off_mixed.data_ptr(), partner.data_ptr(), None, B, len(guided), S, S_G, max(NL), d, st))),
              ("update_all_guided_ms", lambda: hip.check(lib.ditto_guided_update_packed_tags(*head, off_all.data_ptr(), B, S, max(NL), d, 1, st))),
              ("update_unguided_ms", lambda: hip.check(lib.ditto_guided_update_packed_tags(*head, off_all.data_ptr(), B, S, max(NL), d, 0, st))))
        res.update(rounds(ks, args.kernel_iters, 5))
        by = {"update_mixed_ms": (20 * S_G + 12 * (S - S_G)) * d, "update_all_guided_ms": 20 * S * d, "update_unguided_ms": 12 * S * d}
        res["update_bytes"], res["update_guided_rows"] = by, S_G
        for k, _ in ks:
            res[k.replace("_ms", "_TBps")] = by[k] / (res[k] * 1e-3) / 1e12
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
