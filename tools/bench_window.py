#!/usr/bin/env python3
"""Speech infilling at C2 (synthetic weights, B = 32, the lengths of tools/bench_varlen.py — random.Random(2026), N_b in [256, 1024],
T_b in [64, 1024] — as GENERATED frames, a 150-row prefix and a 150-row suffix around each; 25 steps, guidance 5.0, eta 1, seeds), in
ONE process, alternating round by round:
  (a) sample_guided_packed(prompt_lengths=, suffix_lengths=) against the unprompted call on utterances of the same TOTAL lengths
      (G_b + 300 rows): the same forward launch sequence, so (a) should sit inside the unprompted arm's own round-to-round spread;
  (b) the update kernel alone, ditto_guided_update_packed_window against ditto_guided_update_packed on the same buffers (CFG, Philox
      noise): µs and TB/s over 20 B per generated element — the window kernel moves nothing for the 300 context rows per utterance;
  (c) the call WITHOUT suffix_lengths (the lengths of bench_varlen.py, no contexts) against the same call on the PARENT commit's
      library (--parent-lib: a second libditto_hip.so loaded beside this tree's), with the parent a second time as the A/A pair —
      the procedure of tools/bench_interval.py: one model alive at a time, built from a freed device, the order of the three arms
      rotating round by round.
Prints one JSON line and writes it to --out (default profiles/r20_window_bench.json)."""
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
    ap.add_argument("--context", type=int, default=150, help="rows of the prefix and of the suffix of every utterance")
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="libditto_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_window_bench.json"))
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
    B, d, NS, W, K = args.batch, cfg.hidden_dim, args.n_steps, 5.0, args.context
    rng = random.Random(2026)
    GL = [rng.randint(256, 1024) for _ in range(B)]                 # generated frames
    TL = [rng.randint(64, 1024) for _ in range(B)]
    NL = [g + 2 * K for g in GL]                                    # total rows: prefix + generated + suffix
    cu, cg, ct = cumulate(NL), cumulate(GL), cumulate(TL)
    S, SG = cu[-1], cg[-1]

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

    audio = hash_normal((S, d), "bench_window_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_window_text", 2).cuda()
    seeds = torch.arange(B, device="cuda") + 1000
    null = torch.zeros(1, cfg.text_dim, device="cuda")
    res = {"config": "C2", "B": B, "generated_lengths": GL, "text_lengths": TL, "context_rows": K, "rows": S, "generated_rows": SG,
           "rounds": args.rounds, "n_steps": NS, "guidance": W}
    with torch.no_grad():
        def call(g, x, offsets, **kw):
            return lambda: g.sample_guided_packed(text, ct, x, offsets, n_steps=NS, eta=1.0, seeds=seeds, guidance=W, null_text_emb=null,
                                                  **kw)

        # ---------------------------------------------------------------- (c) no suffix_lengths, against the parent library
        arms = [("c_no_suffix_ms", None)]
        if args.parent_lib:
            old = C.CDLL(os.path.abspath(args.parent_lib))
            for name, (r, a) in hip.SYMBOLS.items():
                if hasattr(old, name):
                    getattr(old, name).restype, getattr(old, name).argtypes = r, a
            assert old.ditto_abi_version() == new_lib.ditto_abi_version()
            arms += [("c_parent_ms", old), ("c_parent_again_ms", old)]
        plain_audio = audio[:SG].contiguous()
        runs, outputs = {k: [] for k, _ in arms}, {}
        for rnd in range(args.rounds):
            for k, lib in arms[rnd % len(arms):] + arms[:rnd % len(arms)]:
                g = generator(lib)
                f = call(g, plain_audio, cg)
                runs[k].append(timed(f))
                if rnd == 0:
                    outputs[k] = f().cpu()
                del g, f
                gc.collect()
                torch.cuda.empty_cache()
        for k, v in runs.items():
            res[k], res[k + "_all"] = statistics.median(v), v
        if args.parent_lib:
            assert torch.equal(outputs["c_no_suffix_ms"], outputs["c_parent_ms"])
            p_all = res["c_parent_ms_all"]
            res["c_ratio_over_parent"] = res["c_no_suffix_ms"] / res["c_parent_ms"]
            res["c_parent_again_ratio_over_parent"] = res["c_parent_again_ms"] / res["c_parent_ms"]
            res["c_parent_rounds_max_over_min"] = max(p_all) / min(p_all)
            res["c_inside_parent_spread"] = min(p_all) <= res["c_no_suffix_ms"] <= max(p_all)
        del plain_audio, outputs
        sg = generator()
        # ---------------------------------------------------------------- (a) the windowed call against the unprompted one
        windowed = call(sg, audio, cu, prompt_lengths=[K] * B, suffix_lengths=[K] * B)
        out = windowed()
        for b in range(B):                                          # both contexts come back bit-equal
            assert torch.equal(out[cu[b]:cu[b] + K], audio[cu[b]:cu[b] + K]) and torch.equal(out[cu[b + 1] - K:cu[b + 1]],
                                                                                               audio[cu[b + 1] - K:cu[b + 1]])
        del out
        res.update(rounds([("a_windowed_ms", windowed), ("a_unprompted_same_rows_ms", call(sg, audio, cu))]))
        u_all = res["a_unprompted_same_rows_ms_all"]
        res["a_ratio_over_unprompted"] = res["a_windowed_ms"] / res["a_unprompted_same_rows_ms"]
        res["a_unprompted_rounds_max_over_min"] = max(u_all) / min(u_all)
        res["a_inside_unprompted_spread"] = min(u_all) <= res["a_windowed_ms"] <= max(u_all)
        res["a_windowed_step_ms"], res["a_unprompted_step_ms"] = res["a_windowed_ms"] / NS, res["a_unprompted_same_rows_ms"] / NS
        del sg
        gc.collect()
        torch.cuda.empty_cache()

        # ---------------------------------------------------------------- (b) the update kernel alone
        lib, st = hip.lib(), torch.cuda.current_stream().cuda_stream
        x2 = torch.cat([audio, audio])
        eps2 = hash_normal((2 * S, d), "bench_window_eps2", 5).cuda()
        a, ce, cz, w = (torch.full((B,), v, device="cuda") for v in (0.98, -0.05, 0.1, W))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
        cud, ctx = i32(cu), i32([K] * B)
        head = (x2.data_ptr(), eps2.data_ptr(), None, seeds.data_ptr(), 49, w.data_ptr(), a.data_ptr(), ce.data_ptr(), cz.data_ptr(),
                cud.data_ptr())
        ks = (("update_window_ms", lambda: hip.check(lib.ditto_guided_update_packed_window(*head, ctx.data_ptr(), ctx.data_ptr(), B, S,
                                                                                           max(NL), d, 1, st))),
              ("update_unprompted_ms", lambda: hip.check(lib.ditto_guided_update_packed(*head, B, S, max(NL), d, 1, st))))
        res.update(rounds(ks, args.kernel_iters, 5))
        by = {"update_window_ms": 20 * SG * d, "update_unprompted_ms": 20 * S * d}
        res["update_bytes"] = by
        for k, _ in ks:
            res[k.replace("_ms", "_TBps")] = by[k] / (res[k] * 1e-3) / 1e12
        res["update_time_ratio"] = res["update_window_ms"] / res["update_unprompted_ms"]
        res["update_bytes_ratio"] = by["update_window_ms"] / by["update_unprompted_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
