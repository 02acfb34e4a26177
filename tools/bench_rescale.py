#!/usr/bin/env python3
"""Guidance rescale at C2 (synthetic weights, B = 32, the lengths of tools/bench_varlen.py: random.Random(2026), N_b in [256, 1024],
T_b in [64, 1024]; 25 steps, guidance 5.0, eta 1, seeds), in ONE process, alternating round by round:
  (a) sample_guided_packed WITHOUT the argument against the same call on the PARENT commit's library (--parent-lib: a second
      libditto_hip.so loaded beside this tree's), with a second parent arm as the A/A pair — the same launch sequence, so this
      tree may differ from the parent by no more than the parent's two arms differ from each other.  One model is alive at a time
      and the order of the three arms rotates round by round (tools/bench_interval.py's procedure);
  (b) the two statistics launches alone (ditto_guidance_rescale_packed, phi = 0.7 everywhere): microseconds, bytes read (8 B per
      generated element: c and u) and TB/s, beside the per-utterance-tag update kernel (ditto_guided_update_packed_tags, cfg 1,
      Philox noise: 20 B per element) timed in the same rounds on the same eps2 — and the pair "statistics, then update" as the step
      runs it, where the update re-reads what the statistics just read — and the same two launches with phi = 0, where every workgroup
      leaves before its first load: the floor the two dependent launches cost by themselves;
  (c) the closed call with guidance_rescale = 0.7 against the call without it: ms per call and per step.  The expected difference,
      about 0.1 % of a step, is below the round-to-round spread, which is reported beside it.
Prints one JSON line and writes it to --out (default profiles/r19_rescale_bench.json)."""
import argparse
import gc
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def derive_c(res):
    """(c)'s derived figures from its rounds: the difference per step beside each arm's own round-to-round spread per step; the
    difference counts as resolved only if it exceeds both"""
    NS = res["n_steps"]
    for k in ("c_plain_rounds_spread_per_step_us", "b_scale_sample"):       # fields an earlier version wrote
        res.pop(k, None)
    res["c_rescale_step_ms"], res["c_plain_step_ms"] = res["c_rescale_ms"] / NS, res["c_plain_ms"] / NS
    res["c_difference_per_step_us"] = (res["c_rescale_ms"] - res["c_plain_ms"]) / NS * 1e3
    res["c_rounds_spread_per_step_us"] = {k: (max(res[k + "_all"]) - min(res[k + "_all"])) / NS * 1e3 for k in ("c_rescale_ms", "c_plain_ms")}
    res["c_difference_resolved"] = abs(res["c_difference_per_step_us"]) > max(res["c_rounds_spread_per_step_us"].values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rederive", default=None, metavar="JSON", help="recompute (c)'s derived figures of an earlier result; no GPU")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="libditto_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_rescale_bench.json"))
    args = ap.parse_args()
    if args.rederive:
        res = json.load(open(args.rederive))
        derive_c(res)
        line = json.dumps(res)
        print(line)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return

    import ctypes as C

    import torch
    from ditto_tts_amd import hip
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator
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
            for k, fn in pairs[rnd % len(pairs):] + pairs[:rnd % len(pairs)]:
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
    B, d, NS, W, PHI = args.batch, cfg.hidden_dim, args.n_steps, 5.0, 0.7
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

    audio = hash_normal((S, d), "bench_rescale_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_rescale_text", 2).cuda()
    seeds = torch.arange(B, device="cuda") + 1000
    null = torch.zeros(1, cfg.text_dim, device="cuda")
    res = {"config": "C2", "B": B, "lengths": NL, "text_lengths": TL, "rows": S, "rounds": args.rounds, "n_steps": NS, "guidance": W,
           "phi": PHI, "chunk_quads": hip.RESCALE_CHUNK_QUADS}
    with torch.no_grad():
        def call(g, **kw):
            return lambda: g.sample_guided_packed(text, ct, audio, cu, n_steps=NS, eta=1.0, seeds=seeds, guidance=W, null_text_emb=null,
                                                  **kw)

        # ---------------------------------------------------------------- (a) without the argument, against the parent library
        arms = [("a_no_rescale_ms", None)]
        if args.parent_lib:
            old = C.CDLL(os.path.abspath(args.parent_lib))
            for name, (r, a) in hip.SYMBOLS.items():
                if hasattr(old, name):
                    getattr(old, name).restype, getattr(old, name).argtypes = r, a
            assert old.ditto_abi_version() == new_lib.ditto_abi_version() and not hasattr(old, "ditto_guidance_rescale_packed")
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
            assert torch.equal(outputs["a_no_rescale_ms"], outputs["a_parent_ms"])
            res["a_ratio_over_parent"] = res["a_no_rescale_ms"] / res["a_parent_ms"]
            res["a_parent_again_ratio_over_parent"] = res["a_parent_again_ms"] / res["a_parent_ms"]
            res["a_abs_difference_ms"] = abs(res["a_no_rescale_ms"] - res["a_parent_ms"])
            res["a_parent_arms_abs_difference_ms"] = abs(res["a_parent_again_ms"] - res["a_parent_ms"])
            p_all = res["a_parent_ms_all"] + res["a_parent_again_ms_all"]
            res["a_parent_rounds_min_max_ms"] = [min(p_all), max(p_all)]
            res["a_inside_parent_spread"] = min(p_all) <= res["a_no_rescale_ms"] <= max(p_all)

        # ---------------------------------------------------------------- (c) the rescaled call against the plain one
        sg = generator()
        res.update(rounds([("c_rescale_ms", call(sg, guidance_rescale=PHI)), ("c_plain_ms", call(sg))]))
        derive_c(res)
        eng = sg.ditto_model.engine(torch.device("cuda:0"))
        del sg
        gc.collect()
        torch.cuda.empty_cache()

        # ---------------------------------------------------------------- (b) the statistics launches alone, beside the update
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        x2 = torch.cat([audio, audio])
        eps2 = hash_normal((2 * S, d), "bench_rescale_eps2", 5).cuda()
        a, ce, cz, w, phi = (torch.full((B,), v, device="cuda") for v in (0.98, -0.05, 0.1, W, PHI))
        tags = torch.full((B,), 49, dtype=torch.int32, device="cuda")
        off = torch.tensor(cu + [S + c for c in cu[1:]], dtype=torch.int32, device="cuda")
        scratch = eng.rescale_scratch(B, max(NL))
        coef_out = scratch[:4 * B].view(torch.float32)

        def stats():
            hip.check(lib.ditto_guidance_rescale_packed(eps2.data_ptr(), w.data_ptr(), phi.data_ptr(), ce.data_ptr(), None, off.data_ptr(),
                                                        None, None, B, 0, S, 0, max(NL), d, scratch.data_ptr(), scratch.numel(), st))

        phi0 = torch.zeros(B, device="cuda")

        def floor():    # phi = 0: both launches, every workgroup leaves before its first load — what the two launches cost by themselves
            hip.check(lib.ditto_guidance_rescale_packed(eps2.data_ptr(), w.data_ptr(), phi0.data_ptr(), ce.data_ptr(), None, off.data_ptr(),
                                                        None, None, B, 0, S, 0, max(NL), d, scratch.data_ptr(), scratch.numel(), st))

        def update(coef=ce):
            hip.check(lib.ditto_guided_update_packed_tags(x2.data_ptr(), eps2.data_ptr(), None, seeds.data_ptr(), tags.data_ptr(),
                                                          w.data_ptr(), a.data_ptr(), coef.data_ptr(), cz.data_ptr(), off.data_ptr(), B, S,
                                                          max(NL), d, 1, st))

        def both():
            stats()
            update(coef_out)

        res.update(rounds([("b_statistics_ms", stats), ("b_update_tags_ms", update), ("b_statistics_then_update_ms", both),
                           ("b_statistics_phi_zero_ms", floor)], args.kernel_iters, 5))
        by = {"b_statistics_ms": 8 * S * d, "b_update_tags_ms": 20 * S * d}
        res["b_bytes"] = by
        res["b_statistics_us"], res["b_update_tags_us"] = res["b_statistics_ms"] * 1e3, res["b_update_tags_ms"] * 1e3
        res["b_statistics_TBps"] = by["b_statistics_ms"] / (res["b_statistics_ms"] * 1e-3) / 1e12
        res["b_update_tags_TBps"] = by["b_update_tags_ms"] / (res["b_update_tags_ms"] * 1e-3) / 1e12
        res["b_statistics_phi_zero_us"] = res["b_statistics_phi_zero_ms"] * 1e3
        res["b_statistics_TBps_above_the_launch_floor"] = by["b_statistics_ms"] / ((res["b_statistics_ms"] - res["b_statistics_phi_zero_ms"]) * 1e-3) / 1e12
        res["b_statistics_added_to_update_us"] = (res["b_statistics_then_update_ms"] - res["b_update_tags_ms"]) * 1e3
        res["b_chunks"] = sum(-(-(n * d // 4) // hip.RESCALE_CHUNK_QUADS) for n in NL)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
