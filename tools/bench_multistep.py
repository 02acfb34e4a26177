#!/usr/bin/env python3
"""The second-order multistep step against the strided (DDIM) step at C2 (synthetic weights, B = 32) over the lengths of
tools/bench_varlen.py (random.Random(2026): N_b in [256, 1024], T_b in [64, 1024]), guidance 5.0, in ONE process, alternating round by
round:
  (a) sample_guided_packed(solver="dpmpp2m") per step against (b) solver="ddim" (eta 0, so neither draws noise) on the same batch and
  the same number of steps: the forward is the same launch sequence, so the steps should differ by the update kernel alone;
  the two update kernels alone — ditto_multistep_update_packed at a step with a history (28 B per element: x, eps_c, eps_u, q read,
  both halves and q written) against ditto_guided_update_packed without noise (20 B) — with their bytes and TB/s.
Prints one JSON line (and writes it to --out): per quantity the median of --rounds rounds and every round, the step ratio a / b, and
the DDIM rounds' own spread (max / min) to read that ratio against."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=12)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from ditto_tts_amd import hip
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator
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

    def rounds(pairs, steps, warmup, scale=1.0):
        runs = {k: [] for k, _ in pairs}
        for _ in range(args.rounds):
            for k, fn in pairs:
                runs[k].append(timed(fn, steps, warmup) * scale)
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
    B, d = args.batch, cfg.hidden_dim
    rng = random.Random(2026)
    NL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    cu, ct = cumulate(NL), cumulate(TL)
    S = cu[-1]
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").eval()
    audio = hash_normal((S, d), "bench_multistep_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_multistep_text", 2).cuda()
    seeds = torch.arange(B, device="cuda") + 1000
    res = {"config": "C2", "B": B, "lengths": NL, "text_lengths": TL, "rows": S, "rounds": args.rounds, "n_steps": args.n_steps}
    with torch.no_grad():
        sg = SpeechGenerator(ditto_model=m, device="cuda")
        null = torch.zeros(1, cfg.text_dim, device="cuda")
        kw = dict(n_steps=args.n_steps, guidance=5.0, seeds=seeds, null_text_emb=null)
        fa = lambda: sg.sample_guided_packed(text, ct, audio, cu, solver="dpmpp2m", **kw)      # noqa: E731
        fb = lambda: sg.sample_guided_packed(text, ct, audio, cu, solver="ddim", eta=0.0, **kw)  # noqa: E731
        res.update(rounds((("a_multistep_ms_per_step", fa), ("b_ddim_ms_per_step", fb)), 1, 1, 1.0 / args.n_steps))
        res["step_ratio_a_over_b"] = res["a_multistep_ms_per_step"] / res["b_ddim_ms_per_step"]
        res["ddim_rounds_max_over_min"] = max(res["b_ddim_ms_per_step_all"]) / min(res["b_ddim_ms_per_step_all"])
        res["multistep_rounds_max_over_min"] = max(res["a_multistep_ms_per_step_all"]) / min(res["a_multistep_ms_per_step_all"])
        # the update kernels alone
        lib = hip.lib()
        x2 = torch.cat([audio, audio])
        eps2 = hash_normal((2 * S, d), "bench_multistep_eps2", 5).cuda()
        q = hash_normal((S, d), "bench_multistep_q", 6).cuda()
        cud = torch.tensor(cu, dtype=torch.int32, device="cuda")
        a, ce, w = (torch.full((B,), v, device="cuda") for v in (0.98, -0.05, 5.0))
        st = torch.cuda.current_stream().cuda_stream
        co = hip.MultistepCoef(0.9, 1.02, -0.2, 0.1, -0.03, 0.0, 1, 0)
        first = hip.MultistepCoef(0.9, 1.02, -0.2, 0.1, 0.0, 0.0, 0, 0)
        ms = lambda c: (lambda: hip.check(lib.ditto_multistep_update_packed(  # noqa: E731
            x2.data_ptr(), eps2.data_ptr(), q.data_ptr(), C.byref(c), None, w.data_ptr(), cud.data_ptr(), None, B, S, max(NL), d, 1, st)))
        ks = (("update_multistep_ms", ms(co)), ("update_multistep_first_ms", ms(first)),
              ("update_ddim_ms", lambda: hip.check(lib.ditto_guided_update_packed(
                  x2.data_ptr(), eps2.data_ptr(), None, None, 0, w.data_ptr(), a.data_ptr(), ce.data_ptr(), None, cud.data_ptr(), B, S,
                  max(NL), d, 1, st))))
        res.update(rounds(ks, args.kernel_iters, 5))
        by = {"update_multistep_ms": 28 * S * d, "update_multistep_first_ms": 24 * S * d, "update_ddim_ms": 20 * S * d}
        res["update_bytes"] = by
        for k, _ in ks:
            res[k.replace("_ms", "_TBps")] = by[k] / (res[k] * 1e-3) / 1e12
        res["update_difference_ms"] = res["update_multistep_ms"] - res["update_ddim_ms"]
        res["step_difference_ms"] = res["a_multistep_ms_per_step"] - res["b_ddim_ms_per_step"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
