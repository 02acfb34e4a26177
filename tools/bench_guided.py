#!/usr/bin/env python3
"""The guided strided sampler at C2 (synthetic weights, B = 32, 25 steps, guidance 5.0, eta 1, per-utterance seeds), with the
lengths of tools/bench_varlen.py (random.Random(2026): N_b in [256, 1024], T_b in [64, 1024], padded to N = T = 1024).
ms per denoise step of
  (a) sample_guided on the varlen batch;
  (b) sample_guided dense at the padded lengths;
  (d) one sample_guided call per utterance at its own (N_b, T_b).
(Row (c), sample_latents_strided, was the unfused loop sample_guided replaced; it now runs sample_guided itself and differs from (b)
only in the noise source, so it is no longer timed.)
And the update alone at B = 32, N = 1024: the fused ditto_guided_update (Philox noise, CFG) against the old chain (2 copies into
the doubled batch + cfg_combine + normal_ + linear_update), in us and GB/s on algorithmic bytes.
Prints one JSON line (and writes it to --out).  Timed with HIP events."""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ditto_tts_amd.around import cfg_combine, guided_update_, linear_update_   # noqa: E402
from ditto_tts_amd.config import PRESETS                      # noqa: E402
from ditto_tts_amd.modules import DiTTO                       # noqa: E402
from ditto_tts_amd.sampler import SpeechGenerator             # noqa: E402
from ditto_tts_amd.synth import synthetic_inputs, synthetic_state_dict   # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2, help="timed sampler calls per variant")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = PRESETS["C2"]["cfg"]
    B, N, T, S, G = args.batch, 1024, 1024, args.n_steps, 5.0
    rng = random.Random(2026)
    SL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").eval()
    sg = SpeechGenerator(ditto_model=m, device="cuda")
    x, text, _ = synthetic_inputs(cfg, B, N, T, seed=3)
    x, text = x.cuda(), text.cuda()
    null = torch.zeros(1, T, cfg.text_dim, device="cuda")
    seeds = torch.arange(B, device="cuda") + 1000
    res = {"config": "C2", "B": B, "N_pad": N, "T_pad": T, "n_steps": S, "guidance": G, "eta": 1.0, "speech_lengths": SL,
           "text_lengths": TL, "reps": args.reps}
    kw = dict(n_steps=S, eta=1.0, guidance=G, null_text_emb=null)
    with torch.no_grad():
        res["a_guided_varlen_ms_per_step"] = timed(lambda: sg.sample_guided(text, x, speech_lengths=SL, text_lengths=TL, seeds=seeds,
                                                                            **kw), args.reps, args.warmup) / S
        res["b_guided_dense_ms_per_step"] = timed(lambda: sg.sample_guided(text, x, seeds=seeds, **kw), args.reps, args.warmup) / S
        solo = [(text[b:b + 1, :TL[b]].contiguous(), x[b:b + 1, :SL[b]].contiguous(), seeds[b:b + 1]) for b in range(B)]
        kw1 = dict(n_steps=S, eta=1.0, guidance=G)
        res["d_guided_per_utterance_ms_per_step"] = timed(
            lambda: [sg.sample_guided(t_, x_, seeds=s_, null_text_emb=null[:, :t_.shape[1]], **kw1) for t_, x_, s_ in solo],
            args.reps, args.warmup) / S
        for k in ("a_guided_varlen", "b_guided_dense", "d_guided_per_utterance"):
            res[k + "_utt_steps_per_s"] = B * 1000.0 / res[k + "_ms_per_step"]

        # the update alone (every row valid, then the varlen lengths)
        d = cfg.hidden_dim
        elems = B * N * d
        xs = torch.randn(B, N, d, device="cuda")
        eps2 = torch.randn(2 * B, N, d, device="cuda")
        x2 = torch.empty(2 * B, N, d, device="cuda")
        z = torch.empty(B, N, d, device="cuda")
        a, ce, cz = (torch.full((B,), v, device="cuda") for v in (1.01, -0.3, 0.2))
        w = torch.full((B,), G, device="cuda")
        sl = torch.tensor(SL, dtype=torch.int32, device="cuda")

        def old_chain():
            x2[:B].copy_(xs)
            x2[B:].copy_(xs)
            e = cfg_combine(eps2, G)
            z.normal_()
            linear_update_(xs, e, z, a, ce, cz)

        reps = 50
        res["update_old_chain_us"] = 1000.0 * timed(old_chain, reps, 5)
        res["update_fused_us"] = 1000.0 * timed(lambda: guided_update_(x2, eps2, a, ce, cz, w=w, seeds=seeds, step=7), reps, 5)
        res["update_fused_varlen_us"] = 1000.0 * timed(lambda: guided_update_(x2, eps2, a, ce, cz, w=w, seeds=seeds, step=7,
                                                                              speech_len=sl), reps, 5)
        # algorithmic bytes per element of the B utterances: old = copies 2 x (4 + 4) + cfg_combine (8 + 4) + normal_ 4 +
        # linear_update (12 + 4) = 48; fused = x, c, u read + both halves written = 20
        res["update_old_chain_bytes"] = 48 * elems
        res["update_fused_bytes"] = 20 * elems
        frac = sum(SL) / (B * N)
        res["update_fused_varlen_bytes"] = int(12 * elems * frac + 8 * elems)
        for k in ("update_old_chain", "update_fused", "update_fused_varlen"):
            res[k + "_GBps"] = res[k + "_bytes"] / (res[k + "_us"] * 1e3)
        res["update_fused_fraction_of_6300GBps"] = res["update_fused_GBps"] / 6300.0
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
