#!/usr/bin/env python3
"""What the text gradient and condition dropout cost a packed training step, on tools/bench_train_packed.py's mixed-length C2 batch
(synthetic weights, B = 32: S = 21 145 speech rows, S_T = 17 899 text rows): ms per step — forward + backward + fused AdamW, train
mode — of
  (a) the packed step as it was (frozen text): the launches of the step before the text gradient existed;
  (b) the same step with text_emb.requires_grad: + per layer one pack of the K|V weight rows and one [S_T, 2d] x [2d, text_dim] GEMM
      accumulated into d_text, + the pool path in the tail;
  (c) condition dropout at p_uncond = 0.1 with a learned null embedding [--t0, text_dim] in the optimizer: + the select launch each
      way, the step itself on the effective text (a dropped utterance has --t0 text rows), drop drawn per step from a seeded CPU
      generator.
One process, the three alternating for --rounds rounds after a warm-up of each; medians, every sample and the spread of (a) are
reported — no threshold: the figures are a record.  The arithmetic of the K/V path rides along (text_gemm_flop).
--only a|b|c: just that step, --steps times (for a profiler run of its own).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import random
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ditto_tts_amd.config import PRESETS                      # noqa: E402
from ditto_tts_amd.modules import DiTTO                       # noqa: E402
from ditto_tts_amd.synth import hash_normal, synthetic_state_dict   # noqa: E402


def cu_of(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--t0", type=int, default=32)
    ap.add_argument("--p-uncond", type=float, default=0.1)
    ap.add_argument("--only", default=None, choices=[None, "a", "b", "c"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = PRESETS["C2"]["cfg"]
    B, d = args.batch, cfg.hidden_dim
    rng = random.Random(2026)
    SL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    cu, cu_t = cu_of(SL), cu_of(TL)
    S, S_T = cu[-1], cu_t[-1]
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").train()
    null = torch.nn.Parameter(0.5 * hash_normal((args.t0, cfg.text_dim), "null", 6).cuda())
    opt = torch.optim.AdamW(list(m.parameters()) + [null], lr=1e-5, fused=True)
    xp = hash_normal((S, d), "x", 3).cuda()
    tp = hash_normal((S_T, cfg.text_dim), "text", 4).cuda()
    tp_leaf = tp.clone().requires_grad_()
    noise_p = hash_normal((S, d), "noise", 5).cuda()
    t = torch.tensor([(37 * b + 11) % cfg.diffusion_steps for b in range(B)]).cuda()
    gen = torch.Generator().manual_seed(7)
    dropped = []

    def step_a():
        opt.zero_grad(set_to_none=True)
        F.mse_loss(m.train_forward_packed(xp, cu, tp, cu_t, t, max_seqlen=max(SL), max_text_seqlen=max(TL)), noise_p).backward()
        opt.step()

    def step_b():
        opt.zero_grad(set_to_none=True)
        tp_leaf.grad = None
        F.mse_loss(m.train_forward_packed(xp, cu, tp_leaf, cu_t, t, max_seqlen=max(SL), max_text_seqlen=max(TL)), noise_p).backward()
        opt.step()

    def step_c():
        drop = DiTTO.condition_dropout_mask(B, args.p_uncond, generator=gen)
        dropped.append(int(drop.sum()))
        opt.zero_grad(set_to_none=True)
        F.mse_loss(m.train_forward_packed(xp, cu, tp, cu_t, t, null_text_emb=null, drop=drop, max_seqlen=max(SL),
                                          max_text_seqlen=max(TL)), noise_p).backward()
        opt.step()

    steps = {"a": step_a, "b": step_b, "c": step_c}
    res = {"config": "C2", "B": B, "S": S, "S_T": S_T, "T0": args.t0, "p_uncond": args.p_uncond, "rounds": args.rounds,
           "text_gemm_flop": cfg.num_layers * 2 * S_T * 2 * d * cfg.text_dim, "d_text_bytes": S_T * cfg.text_dim * 4}
    if args.only:
        for _ in range(args.warmup):
            steps[args.only]()
        torch.cuda.synchronize()
        res[f"{args.only}_ms"] = statistics.median(timed(steps[args.only]) for _ in range(args.steps))
        res["steps_run"] = args.warmup + args.steps
    else:
        for _ in range(args.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        del dropped[:]
        ts = {k: [] for k in steps}
        for _ in range(args.rounds):
            for k, fn in steps.items():
                ts[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ts.items()}
        res.update({"a_frozen_text_ms": med["a"], "b_text_grad_ms": med["b"], "c_cond_dropout_ms": med["c"],
                    "a_all_ms": ts["a"], "b_all_ms": ts["b"], "c_all_ms": ts["c"], "a_spread_ms": max(ts["a"]) - min(ts["a"]),
                    "b_minus_a_ms": med["b"] - med["a"], "c_minus_a_ms": med["c"] - med["a"], "c_dropped_per_step": list(dropped)})
        assert tp_leaf.grad is not None and null.grad is not None
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
