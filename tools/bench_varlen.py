#!/usr/bin/env python3
"""Variable-length batches at C2 (synthetic weights, B = 32): ms per denoise step and utterance-steps/s of
  (a) one varlen batch: N_b uniform in [256, 1024], T_b uniform in [64, 1024] (fixed seed), padded to N = T = 1024;
  (b) one call per utterance at its own (N_b, T_b) — the only exact option without lengths;
  (c) the dense B = 32, N = T = 1024 step.
Prints one JSON line (and writes it to --out).  Timed with HIP events over --steps steps after --warmup."""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ditto_tts_amd.config import PRESETS                      # noqa: E402
from ditto_tts_amd.modules import DiTTO                       # noqa: E402
from ditto_tts_amd.synth import synthetic_inputs, synthetic_state_dict   # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = PRESETS["C2"]["cfg"]
    B, N, T = args.batch, 1024, 1024
    rng = random.Random(2026)
    SL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").eval()
    x, text, t = synthetic_inputs(cfg, B, N, T, seed=3)
    x, text, t = x.cuda(), text.cuda(), t.cuda()
    eng = m.engine()
    res = {"config": "C2", "B": B, "N_pad": N, "T_pad": T, "speech_lengths": SL, "text_lengths": TL, "steps": args.steps}
    with torch.no_grad():
        cond_v = eng.prepare_text(text, N, text_lengths=TL)
        sl = torch.tensor(SL, dtype=torch.int32, device="cuda")
        res["a_varlen_ms"] = timed(lambda: eng.forward(x, cond_v, t, speech_lengths=sl), args.steps, args.warmup)
        solo = [(x[b:b + 1, :SL[b]].contiguous(), eng.prepare_text(text[b:b + 1, :TL[b]].contiguous(), SL[b]), t[b:b + 1])
                for b in range(B)]
        res["b_per_utterance_ms"] = timed(lambda: [eng.forward(xs, cs, ts) for xs, cs, ts in solo], args.steps, args.warmup)
        cond_d = eng.prepare_text(text, N)
        res["c_dense_ms"] = timed(lambda: eng.forward(x, cond_d, t), args.steps, args.warmup)
    for k in ("a_varlen", "b_per_utterance", "c_dense"):
        res[k + "_utt_steps_per_s"] = B * 1000.0 / res[k + "_ms"]
    res["self_attn_work_a_over_c"] = sum(n * n for n in SL) / (B * N * N)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
