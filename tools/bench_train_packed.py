#!/usr/bin/env python3
"""Training on a mixed-length batch at C2 (synthetic weights, B = 32, the lengths of tools/bench_varlen.py: S = 21 145 speech rows,
S_T = 17 899 text rows): ms per training step — forward + backward + fused AdamW, train mode — of
  (a) the packed step (DiTTO.train_forward_packed): no padding row exists;
  (b) the dense step on the same batch padded to N = T = 1024 (DiTTO.forward under autograd: it computes the PADDED function, so it
      is a cost baseline, not a parity one);
  (c) one dense call per utterance at its own (N_b, T_b), gradients accumulated, one optimizer step — the exact option without (a).
One process, (a) / (b) alternating for --rounds rounds after a warm-up of every shape; medians and the spread of (b) are reported.
Parity rides along: the forward of three utterances of the batch (eval mode) against their solo dense training forward, rel-L2.
--only a: just the packed step, --steps times (for a profiler run of its own).  Prints one JSON line (and writes it to --out); exits
non-zero when the parity fails, (a) is not below (b) by more than (b)'s spread, or (a) is not below (c)."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--only", default=None, choices=[None, "a"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = PRESETS["C2"]["cfg"]
    B, N, T, d = args.batch, 1024, 1024, cfg.hidden_dim
    rng = random.Random(2026)
    SL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    cu, cu_t = cu_of(SL), cu_of(TL)
    S, S_T = cu[-1], cu_t[-1]
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-5, fused=True)
    xp = hash_normal((S, d), "x", 3).cuda()
    tp = hash_normal((S_T, cfg.text_dim), "text", 4).cuda()
    noise_p = hash_normal((S, d), "noise", 5).cuda()
    t = torch.tensor([(37 * b + 11) % cfg.diffusion_steps for b in range(B)]).cuda()
    x = torch.zeros(B, N, d, device="cuda"); text = torch.zeros(B, T, cfg.text_dim, device="cuda"); noise = torch.zeros(B, N, d, device="cuda")
    for b in range(B):
        x[b, :SL[b]] = xp[cu[b]:cu[b + 1]]; noise[b, :SL[b]] = noise_p[cu[b]:cu[b + 1]]
        text[b, :TL[b]] = tp[cu_t[b]:cu_t[b + 1]]
    solo = [(x[b:b + 1, :SL[b]].contiguous(), text[b:b + 1, :TL[b]].contiguous(), t[b:b + 1], noise[b:b + 1, :SL[b]].contiguous())
            for b in range(B)]

    def step_a():
        opt.zero_grad(set_to_none=True)
        F.mse_loss(m.train_forward_packed(xp, cu, tp, cu_t, t, max_seqlen=max(SL), max_text_seqlen=max(TL)), noise_p).backward()
        opt.step()

    def step_b():
        opt.zero_grad(set_to_none=True)
        F.mse_loss(m(x, text, t), noise).backward()
        opt.step()

    def step_c():
        opt.zero_grad(set_to_none=True)
        for xs, ts, tt, ns in solo:
            (F.mse_loss(m(xs, ts, tt), ns, reduction="sum") / (S * d)).backward()
        opt.step()

    res = {"config": "C2", "B": B, "S": S, "S_T": S_T, "N_pad": N, "T_pad": T, "rounds": args.rounds,
           "row_ratio": S / (B * N), "text_row_ratio": S_T / (B * T),
           "self_attn_work_ratio": sum(n * n for n in SL) / (B * N * N),
           "cross_attn_work_ratio": sum(n * k for n, k in zip(SL, TL)) / (B * N * T)}
    if args.only == "a":
        for _ in range(args.warmup):
            step_a()
        torch.cuda.synchronize()
        res["a_packed_ms"] = statistics.median(timed(step_a) for _ in range(args.steps))
    else:
        # parity at the timed size: three utterances' packed forward against their solo dense training forward (eval mode)
        m.eval()
        with torch.enable_grad():
            full = m.train_forward_packed(xp, cu, tp, cu_t, t).detach()
            rel = {}
            for b in (0, B // 2, B - 1):
                xs, ts, tt, _ = solo[b]
                want = m(xs, ts, tt).detach()[0]
                got = full[cu[b]:cu[b + 1]]
                rel[str(b)] = float((got - want).norm() / want.norm())
        res["parity_rel_l2"] = rel
        res["parity_ok"] = all(v <= 2e-2 for v in rel.values())
        m.train()
        for _ in range(args.warmup):
            step_a(); step_b()
        step_c()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(step_a)); tb.append(timed(step_b))
        tc = [timed(step_c) for _ in range(max(2, args.rounds // 2))]
        res.update({"a_packed_ms": statistics.median(ta), "b_padded_dense_ms": statistics.median(tb),
                    "c_per_utterance_ms": statistics.median(tc), "a_all_ms": ta, "b_all_ms": tb, "c_all_ms": tc,
                    "b_spread_ms": max(tb) - min(tb)})
        res["a_over_b"] = res["a_packed_ms"] / res["b_padded_dense_ms"]
        res["a_below_b_by_more_than_b_spread"] = res["b_padded_dense_ms"] - res["a_packed_ms"] > res["b_spread_ms"]
        res["a_below_c"] = res["a_packed_ms"] < res["c_per_utterance_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    failed = [k for k in ("parity_ok", "a_below_b_by_more_than_b_spread", "a_below_c") if res.get(k) is False]
    if failed:
        sys.exit("bench_train_packed: " + ", ".join(failed) + " is false")


if __name__ == "__main__":
    main()
