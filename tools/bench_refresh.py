#!/usr/bin/env python3
"""Reuse of the guidance direction at C2 (synthetic weights, B = 32, the lengths of tools/bench_varlen.py: random.Random(2026), N_b in
[256, 1024], T_b in [64, 1024]; 25 steps, guidance 5.0, eta 1, seeds), in ONE process, HIP events, alternating round by round:
  (a) one reuse step (ditto_guided_step_packed_reuse_opts in LOAD mode, mirror on) against one unguided step (the existing
      ditto_guided_step_packed_opts with cfg 0) on the same batch, state and conditioning — and against the per-step time of the whole
      unguided loop, sample_guided_packed(guidance=None) / 25, the parent's yardstick.  Beside them a refresh step (STORE) against the
      existing guided step, and the two update kernels alone (LOAD against the unguided update: the additional 4 B per generated
      element), in µs and TB/s;
  (b) the whole 25-step call at guidance_refresh = 1, 2, 3, 5 against the row-count model of the forward work: (25 + refreshes) / 50
      of the k = 1 call (asymptotically 1, 3/4, 2/3, 3/5);
  (c) with prediction="v" (the eps loop of the synthetic weights blows up to 5e5), the rel-L2 of the final latents at k = 2, 3, 5
      against k = 1.  Synthetic weights: this says how far the trajectories of THIS network drift, nothing about speech.
Medians with [min, max] over --rounds.  Prints one JSON line and writes it to --out (default profiles/refresh_bench.json)."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_bench.json"))
    args = ap.parse_args()

    import torch
    from ditto_tts_amd import hip
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator, refresh_plan
    from ditto_tts_amd.synth import hash_normal, synthetic_state_dict

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
        for rnd in range(args.rounds):
            order = pairs[rnd % len(pairs):] + pairs[:rnd % len(pairs)]          # the order rotates round by round
            for k, fn in order:
                runs[k].append(timed(fn, steps, warmup))
        out = {}
        for k, v in runs.items():
            out[k] = statistics.median(v)
            out[k + "_min_max"] = [min(v), max(v)]
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
    S, N = cu[-1], max(NL)
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    sg = SpeechGenerator(ditto_model=m.to("cuda").eval(), device="cuda")
    eng = sg.ditto_model.engine(torch.device("cuda:0"))
    audio = hash_normal((S, d), "bench_refresh_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_refresh_text", 2).cuda()
    seeds = torch.arange(B, device="cuda") + 1000
    null = torch.zeros(1, cfg.text_dim, device="cuda")
    res = {"config": "C2", "B": B, "lengths": NL, "text_lengths": TL, "rows": S, "rounds": args.rounds, "n_steps": NS, "guidance": W,
           "weights": "synthetic", "trained_model_run": False, "measured_on": "one MI355X, one process"}
    with torch.no_grad():
        # ---------------------------------------------------------------- (a) one step of each kind
        cond2 = eng.prepare_text_packed(torch.cat([text, null.expand_as(text)]).contiguous(), ct + [ct[-1] + c for c in ct[1:]])
        cond1 = eng.prepare_text_packed(text, ct)
        off2, off1 = eng.guided_offsets_packed(cu, S, N, True), eng.guided_offsets_packed(cu, S, N, False)
        x2 = torch.cat([audio, audio]).contiguous()
        keep = x2.clone()
        delta = hash_normal((S, d), "bench_refresh_delta", 3).cuda() * 0.01
        a, ce, cz, w = (torch.full((B,), v, device="cuda") for v in (0.98, -0.05, 0.1, W))
        t2, t1 = torch.full((2 * B,), 25, device="cuda"), torch.full((B,), 25, device="cuda")      # a timestep of the 50-row table
        kw = dict(seeds=seeds, step=25)

        def fresh(fn):                                       # every timed step starts from the same state (one 2S x d copy in the timing
            def run():                                       # of each arm alike)
                x2.copy_(keep)
                fn()
            return run

        steps = [("a_reuse_step_ms", fresh(lambda: eng.guided_step_packed_reuse_(x2[:S], cond1, t1, B, delta, a, ce, cz, w, hip.REUSE_LOAD,
                                                                                 mirror=True, offsets=off1, **kw))),
                 ("a_unguided_step_ms", fresh(lambda: eng.guided_step_packed_(x2[:S], cond1, t1, B, a, ce, cz, offsets=off1, **kw))),
                 ("a_refresh_step_ms", fresh(lambda: eng.guided_step_packed_reuse_(x2, cond2, t2, B, delta, a, ce, cz, w, hip.REUSE_STORE,
                                                                                   offsets=off2, **kw))),
                 ("a_guided_step_ms", fresh(lambda: eng.guided_step_packed_(x2, cond2, t2, B, a, ce, cz, w=w, offsets=off2, **kw))),
                 ("a_state_copy_ms", fresh(lambda: None))]
        res.update(rounds(steps, args.step_iters, 2))
        for k in ("a_reuse_step_ms", "a_unguided_step_ms", "a_refresh_step_ms", "a_guided_step_ms"):
            res[k.replace("_ms", "_net_ms")] = res[k] - res["a_state_copy_ms"]
        res["a_reuse_over_unguided_step"] = res["a_reuse_step_net_ms"] / res["a_unguided_step_net_ms"]
        res["a_refresh_over_guided_step"] = res["a_refresh_step_net_ms"] / res["a_guided_step_net_ms"]

        # the update kernels alone
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        eps2 = hash_normal((2 * S, d), "bench_refresh_eps2", 5).cuda()
        cud = off1[0]
        head = lambda e: (x2.data_ptr(), e.data_ptr())                                     # noqa: E731
        tail = (None, seeds.data_ptr(), 500, w.data_ptr(), a.data_ptr(), ce.data_ptr(), cz.data_ptr(), cud.data_ptr())
        reuse = lambda mode, mirror: lambda: hip.check(lib.ditto_guided_update_packed_reuse(     # noqa: E731
            *head(eps2), delta.data_ptr(), *tail, None, None, B, S, N, d, mode, mirror, st))
        plain = lambda cfg_on: lambda: hip.check(lib.ditto_guided_update_packed(                 # noqa: E731
            *head(eps2), None, seeds.data_ptr(), 500, w.data_ptr() if cfg_on else None, a.data_ptr(), ce.data_ptr(), cz.data_ptr(),
            cud.data_ptr(), B, S, N, d, cfg_on, st))
        ks = [("update_load_ms", reuse(hip.REUSE_LOAD, 0)), ("update_load_mirror_ms", reuse(hip.REUSE_LOAD, 1)),
              ("update_unguided_ms", plain(0)), ("update_store_ms", reuse(hip.REUSE_STORE, 0)), ("update_guided_ms", plain(1))]
        res.update(rounds(ks, args.kernel_iters, 5))
        by = {"update_load_ms": 16, "update_load_mirror_ms": 20, "update_unguided_ms": 12, "update_store_ms": 24, "update_guided_ms": 20}
        res["update_bytes_per_element"] = by
        for k, _ in ks:
            res[k.replace("_ms", "_TBps")] = by[k] * S * d / (res[k] * 1e-3) / 1e12
        res["update_load_minus_unguided_ms"] = res["update_load_mirror_ms"] - res["update_unguided_ms"]
        x2.copy_(keep)
        del eps2

        # ---------------------------------------------------------------- (b) the whole call
        def call(**kw2):
            gkw = dict(guidance=W, null_text_emb=null) if kw2.pop("guided", True) else {}
            return lambda: sg.sample_guided_packed(text, ct, audio, cu, n_steps=NS, eta=1.0, seeds=seeds, **gkw, **kw2)

        KS = (1, 2, 3, 5)
        res.update(rounds([(f"b_k{k}_ms", call(guidance_refresh=k)) for k in KS] + [("b_unguided_ms", call(guided=False))]))
        res["b_unguided_loop_step_ms"] = res["b_unguided_ms"] / NS
        res["b_unguided_loop_step_ms_min_max"] = [v / NS for v in res["b_unguided_ms_min_max"]]
        extra = res["update_load_mirror_ms"] - res["update_unguided_ms"]
        lo, hi = res["a_unguided_step_ms_min_max"]
        res["a_reuse_step_expected_at_most_ms"] = hi + max(extra, 0.0)
        res["a_reuse_step_inside_unguided_spread_plus_extra_bytes"] = res["a_reuse_step_ms"] <= hi + max(extra, 0.0)
        for k in KS:
            n_refresh = refresh_plan([True] * NS, k)[0].count("refresh")
            res[f"b_k{k}_refreshes"] = n_refresh
            res[f"b_k{k}_over_k1"] = res[f"b_k{k}_ms"] / res["b_k1_ms"]
            res[f"b_k{k}_row_model"] = (NS + n_refresh) / (2 * NS)
            res[f"b_k{k}_row_model_asymptotic"] = (k + 1) / (2 * k)
            res[f"b_k{k}_step_model_ms"] = n_refresh * res["b_k1_ms"] / NS + (NS - n_refresh) * res["b_unguided_ms"] / NS

        # ---------------------------------------------------------------- (c) how far the k-step trajectories drift (v-prediction)
        base = call(guidance_refresh=1, prediction="v")().double()
        res["c_prediction"] = "v"
        res["c_k1_abs_max"] = float(base.abs().max())
        for k in KS[1:]:
            out = call(guidance_refresh=k, prediction="v")().double()
            res[f"c_k{k}_rel_l2_vs_k1"] = float((out - base).norm() / base.norm())
            assert torch.isfinite(out).all()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
