#!/usr/bin/env python3
"""ditto_span_vloss_window (the v objective's span loss) beside ditto_span_mse_window at the mixed-length C2 batch of bench_varlen.py
(B = 32, N_b uniform in [256, 1024], fixed seed; d = 768) with P_b = N_b / 8 prompt rows and Q_b = N_b / 16 suffix rows: microseconds
per call of the C entry (the kernel and the finish launch) and the rate its byte count gives — 8 / 12 B per generated element for
the MSE (seeded / with a noise buffer), 12 / 16 B for the v loss, 4 B per context element (the zero of its gradient).  One process,
HIP events around --steps launches after --warmup, --rounds rounds with the four entries alternating.  Prints one JSON line (and
writes it to --out)."""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ditto_tts_amd import hip                                 # noqa: E402
from ditto_tts_amd.config import PRESETS                      # noqa: E402


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
    return a.elapsed_time(b) / steps * 1e3                    # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    d, B = PRESETS["C2"]["cfg"].hidden_dim, 32
    rng = random.Random(2026)
    SL = [rng.randint(256, 1024) for _ in range(B)]
    cu = [0]
    for n in SL:
        cu.append(cu[-1] + n)
    S, max_N = cu[-1], max(SL)
    P, Q = [n // 8 for n in SL], [n // 16 for n in SL]
    gen = S - sum(P) - sum(Q)
    lib = hip.lib()
    pred, x0, z = (torch.randn(S, d, device="cuda") for _ in range(3))
    ca, cs, lw = (torch.rand(B, device="cuda") for _ in range(3))
    seeds = torch.arange(B, device="cuda", dtype=torch.int64)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    cud, pld, qld = i32(cu), i32(P), i32(Q)
    grad, loss = torch.empty_like(pred), torch.empty(1, device="cuda")
    part = torch.empty(B * min(1024, (max_N * d // 4 + 255) // 256), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    tail = (gen * d, grad.data_ptr(), loss.data_ptr(), part.data_ptr(), part.numel() * 4, B, S, max_N, d, st)

    def mse(noise, sd):
        return lambda: hip.check(lib.ditto_span_mse_window(pred.data_ptr(), noise, sd, 1, cud.data_ptr(), pld.data_ptr(), qld.data_ptr(),
                                                           *tail))

    def vloss(noise, sd):
        return lambda: hip.check(lib.ditto_span_vloss_window(pred.data_ptr(), x0.data_ptr(), noise, sd, 1, ca.data_ptr(), cs.data_ptr(),
                                                             lw.data_ptr(), cud.data_ptr(), pld.data_ptr(), qld.data_ptr(), *tail))

    res = {"config": "C2", "B": B, "S": S, "d": d, "generated_rows": gen, "steps": args.steps, "rounds": args.rounds}
    arms = (("mse_seeds", mse(None, seeds.data_ptr()), 8), ("vloss_seeds", vloss(None, seeds.data_ptr()), 12),
            ("mse_noise", mse(z.data_ptr(), None), 12), ("vloss_noise", vloss(z.data_ptr(), None), 16))
    for _ in range(args.rounds):
        for name, fn, bytes_el in arms:
            us = timed(fn, args.steps, args.warmup)
            traffic = gen * d * bytes_el + (S - gen) * d * 4
            res.setdefault(name, []).append({"us": round(us, 2), "GBps": round(traffic / us / 1e3, 1)})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
