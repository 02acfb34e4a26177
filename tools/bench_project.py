#!/usr/bin/env python3
"""Projected guidance (APG) at C2 (synthetic weights, B = 32, the lengths of tools/bench_varlen.py: random.Random(2026), N_b in
[256, 1024], T_b in [64, 1024]; 25 steps, guidance 5.0, eta 1, seeds), in ONE process, alternating round by round — the procedure of
tools/bench_rescale.py:
  (a) sample_guided_packed WITHOUT the keywords against the same call on the PARENT commit's library (--parent-lib: a second
      libditto_hip.so loaded beside this tree's), with a second parent arm as the A/A pair.  The guarantee for a caller who does not
      use the feature is the machine-code identity of every existing kernel (tools/asm_identity.py); this timing only confirms it
      within the parent's own round-to-round spread.  One model is alive at a time and the order of the arms rotates;
  (b) the two project launches alone (ditto_guidance_project_packed: the direction + partial sums, and the finish) with use_prev = 0
      (x, c, u read, m' written: 16 B per generated element) and use_prev = 1 (+ m read: 20 B), and the new update alone
      (ditto_guided_update_packed_project, Philox noise: x, c, m' read, both halves written, 20 B), as microseconds, bytes and TB/s,
      beside the existing CFG update (ditto_guided_update_packed, cfg 1, Philox: 20 B) timed in the same rounds on the same buffers;
      and "project, then update" as the step runs them;
  (c) the closed call with guidance_projection = 0.5, guidance_norm_threshold = 2.0, guidance_momentum = -0.5 against the plain one:
      ms per call and per step, beside each arm's round-to-round spread.
Prints one JSON line and writes it to --out (default profiles/project_bench.json)."""
import argparse
import gc
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
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="libditto_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_bench.json"))
    args = ap.parse_args()

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
    B, d, NS, W = args.batch, cfg.hidden_dim, args.n_steps, 5.0
    PJ = dict(guidance_projection=0.5, guidance_norm_threshold=2.0, guidance_momentum=-0.5)
    rng = random.Random(2026)
    NL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    cu, ct = cumulate(NL), cumulate(TL)
    S = cu[-1]
    state = synthetic_state_dict(cfg, seed=1)
    new_lib = hip.lib()

    def generator():
        """a generator whose engine is bound to the library hip.lib() gives at this moment"""
        m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
        m.load_state_dict(state)
        g = SpeechGenerator(ditto_model=m.to("cuda").eval(), device="cuda")
        assert g.ditto_model.engine(torch.device("cuda:0")).lib is hip.lib()
        return g

    audio = hash_normal((S, d), "bench_project_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_project_text", 2).cuda()
    seeds = torch.arange(B, device="cuda") + 1000
    null = torch.zeros(1, cfg.text_dim, device="cuda")
    res = {"config": "C2", "B": B, "lengths": NL, "text_lengths": TL, "rows": S, "rounds": args.rounds, "n_steps": NS, "guidance": W,
           "projection": PJ, "chunk_quads": hip.RESCALE_CHUNK_QUADS}
    with torch.no_grad():
        def call(g, **kw):
            return lambda: g.sample_guided_packed(text, ct, audio, cu, n_steps=NS, eta=1.0, seeds=seeds, guidance=W, null_text_emb=null,
                                                  **kw)

        # ---------------------------------------------------------------- (a) without the keywords, against the parent library
        arms = [("a_no_projection_ms", None)]
        if args.parent_lib:
            old = C.CDLL(os.path.abspath(args.parent_lib))
            for name, (r, a) in hip.SYMBOLS.items():
                if hasattr(old, name):
                    getattr(old, name).restype, getattr(old, name).argtypes = r, a
            assert old.ditto_abi_version() == new_lib.ditto_abi_version() and not hasattr(old, "ditto_guidance_project_packed")
            arms += [("a_parent_ms", old), ("a_parent_again_ms", old)]
        runs, outputs = {k: [] for k, _ in arms}, {}
        for rnd in range(args.rounds):
            for k, lib in arms[rnd % len(arms):] + arms[:rnd % len(arms)]:
                # the arm's library stands in for hip.lib() while its model is built AND while it runs: the engine keeps the library it
                # was built with, but the step entries are called by name through hip.call, which asks hip.lib() at every call
                hip._lib = lib or new_lib
                try:
                    g = generator()
                    f = call(g)
                    runs[k].append(timed(f))
                    if rnd == 0:
                        outputs[k] = f().cpu()
                    del g, f
                finally:
                    hip._lib = new_lib
                gc.collect()
                torch.cuda.empty_cache()
        for k, v in runs.items():
            res[k], res[k + "_all"] = statistics.median(v), v
        if args.parent_lib:
            assert torch.equal(outputs["a_no_projection_ms"], outputs["a_parent_ms"])
            res["a_outputs_bit_equal_to_parent"] = True
            res["a_ratio_over_parent"] = res["a_no_projection_ms"] / res["a_parent_ms"]
            res["a_parent_again_ratio_over_parent"] = res["a_parent_again_ms"] / res["a_parent_ms"]
            p_all = res["a_parent_ms_all"] + res["a_parent_again_ms_all"]
            res["a_parent_rounds_min_max_ms"] = [min(p_all), max(p_all)]
            res["a_inside_parent_spread"] = min(p_all) <= res["a_no_projection_ms"] <= max(p_all)

        # ---------------------------------------------------------------- (c) the projected call against the plain one
        sg = generator()
        res.update(rounds([("c_projected_ms", call(sg, **PJ)), ("c_plain_ms", call(sg))]))
        res["c_projected_step_ms"], res["c_plain_step_ms"] = res["c_projected_ms"] / NS, res["c_plain_ms"] / NS
        res["c_difference_per_step_us"] = (res["c_projected_ms"] - res["c_plain_ms"]) / NS * 1e3
        res["c_rounds_spread_per_step_us"] = {k: (max(res[k + "_all"]) - min(res[k + "_all"])) / NS * 1e3
                                              for k in ("c_projected_ms", "c_plain_ms")}
        res["c_difference_resolved"] = abs(res["c_difference_per_step_us"]) > max(res["c_rounds_spread_per_step_us"].values())
        eng = sg.ditto_model.engine(torch.device("cuda:0"))
        del sg
        gc.collect()
        torch.cuda.empty_cache()

        # ---------------------------------------------------------------- (b) the project launches and the new update alone
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        x2 = torch.cat([audio, audio])
        eps2 = hash_normal((2 * S, d), "bench_project_eps2", 5).cuda()
        direction = hash_normal((S, d), "bench_project_dir", 6).cuda()
        a, ce, cz, w = (torch.full((B,), v, device="cuda") for v in (0.98, -0.05, 0.1, W))
        off = torch.tensor(cu + [S + c for c in cu[1:]], dtype=torch.int32, device="cuda")
        scratch = eng.project_scratch(B, max(NL))
        proj = {}
        for use_prev in (0, 1):
            t = torch.zeros(B, 8)
            t[:, :6] = torch.tensor([1.9, -1.6, W, PJ["guidance_projection"], PJ["guidance_norm_threshold"], PJ["guidance_momentum"]])
            t.view(torch.int32)[:, 6] = use_prev
            proj[use_prev] = t.cuda()
        rows = dict(cu=off.data_ptr(), prompt_len=None, suffix_len=None, B=B, S=S, max_N=max(NL), d=d, stream=st)

        def project(use_prev):
            # beta = -0.5 with |dd| ~ 1: the direction's size settles (sum of |beta|^k), so use_prev = 1 can run any number of times
            return lambda: hip.check(hip.call("ditto_guidance_project_packed", x2=x2.data_ptr(), eps2=eps2.data_ptr(), dir=direction.data_ptr(),
                                              proj=proj[use_prev].data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(),
                                              **rows))

        def update_project():
            hip.check(hip.call("ditto_guided_update_packed_project", x2=x2.data_ptr(), eps2=eps2.data_ptr(), dir=direction.data_ptr(),
                               pcoef=scratch.data_ptr(), noise=None, seeds=seeds.data_ptr(), step=49, tags=None, a=a.data_ptr(),
                               ce=ce.data_ptr(), cz=cz.data_ptr(), **rows))

        def update_cfg():
            hip.check(lib.ditto_guided_update_packed(x2.data_ptr(), eps2.data_ptr(), None, seeds.data_ptr(), 49, w.data_ptr(), a.data_ptr(),
                                                     ce.data_ptr(), cz.data_ptr(), off.data_ptr(), B, S, max(NL), d, 1, st))

        def both():
            project(1)()
            update_project()

        # |a| < 1 and small ce, cz: x2 stays bounded however often the updates run in place
        res.update(rounds([("b_project_first_ms", project(0)), ("b_project_ms", project(1)), ("b_update_project_ms", update_project),
                           ("b_update_cfg_ms", update_cfg), ("b_project_then_update_ms", both)], args.kernel_iters, 5))
        assert torch.isfinite(x2).all() and torch.isfinite(direction).all()
        by = {"b_project_first_ms": 16 * S * d, "b_project_ms": 20 * S * d, "b_update_project_ms": 20 * S * d, "b_update_cfg_ms": 20 * S * d}
        res["b_bytes"] = by
        for k, n in by.items():
            res[k[:-3] + "_us"] = res[k] * 1e3
            res[k[:-3] + "_TBps"] = n / (res[k] * 1e-3) / 1e12
            res[k[:-3] + "_rounds_min_max_us"] = [min(res[k + "_all"]) * 1e3, max(res[k + "_all"]) * 1e3]
        res["b_project_then_update_us"] = res["b_project_then_update_ms"] * 1e3
        res["b_added_to_the_cfg_update_us"] = (res["b_project_then_update_ms"] - res["b_update_cfg_ms"]) * 1e3
        res["b_chunks"] = sum(-(-(n * d // 4) // hip.RESCALE_CHUNK_QUADS) for n in NL)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
