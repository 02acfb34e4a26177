#!/usr/bin/env python3
"""Packed batches at C2 (synthetic weights, B = 32) with the lengths of tools/bench_varlen.py (random.Random(2026): N_b in
[256, 1024], T_b in [64, 1024]; the padded forms at N = T = 1024).  In ONE process, alternating round by round:
  (a) DiTTO forward over the packed batch (engine.forward_packed), (b) the padded varlen forward (forward(speech_lengths=)),
  (c) the dense forward at B = 32, N = T = 1024;
  (d) sample_guided_packed per step against (e) sample_guided(speech_lengths=, text_lengths=) per step (25 steps, guidance 5.0,
  eta 1, per-utterance seeds).
Prints one JSON line (and writes it to --out): the median of --rounds rounds of each, the ratios a / b and d / e, the row fractions.
  --only packed|varlen   one forward variant only, --steps times (for a rocprofv3 --kernel-trace --stats run of its own)
  --split A.csv B.csv    per kernel class totals (ms per forward, --steps forwards each) of two such runs' kernel_stats.csv"""
import argparse
import csv
import json
import os
import random
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = [("attention", r"attn64"), ("gemm_qkv_rope", r"gemm(256|128|128_deep)_kernel<(2|9)[,>]"),
           ("gemm_gated_mlp", r"gemm(256|128|128_deep)_kernel<3[,>]"), ("gemm_full_row", r"gemm_fr(d|64)?_kernel"),
           ("gemm_ln_qproj", r"gemm_lnq"), ("gemm_other", r"gemm"), ("layernorm_adaln", r"ln_kernel"),
           ("splitk_finish", r"splitk"), ("row_map", r"packed_row_map"), ("zero_rows", r"zero_rows")]


def kernel_class(name):
    for cls, pat in CLASSES:
        if re.search(pat, name):
            return cls
    return "other"


def split(paths, steps):
    out = {}
    for tag, p in zip(("a_packed", "b_varlen"), paths):
        tot = {}
        with open(p) as f:
            for row in csv.DictReader(f):
                c = kernel_class(row["Name"])
                tot[c] = tot.get(c, 0.0) + float(row["TotalDurationNs"]) / 1e6 / steps
        out[tag] = {k: round(v, 4) for k, v in sorted(tot.items())}
        out[tag]["total"] = round(sum(tot.values()), 4)
    out["ratio_a_over_b"] = {k: round(out["a_packed"].get(k, 0.0) / v, 4) for k, v in out["b_varlen"].items() if v > 0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="forwards per timed run")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of (a, b, c)")
    ap.add_argument("--guided-rounds", type=int, default=2, help="alternating rounds of (d, e), one sampler call each")
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--only", choices=["packed", "varlen"], default=None)
    ap.add_argument("--split", nargs=2, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.split:
        line = json.dumps(split(args.split, args.steps))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    import torch
    from ditto_tts_amd import varlen
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator
    from ditto_tts_amd.synth import synthetic_inputs, synthetic_state_dict

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
    xp, cu = varlen.pack(x, SL)
    tp, ct = varlen.pack(text, TL)
    eng = m.engine()
    res = {"config": "C2", "B": B, "N_pad": N, "T_pad": T, "speech_lengths": SL, "text_lengths": TL, "steps": args.steps,
           "rounds": args.rounds, "speech_rows": int(xp.shape[0]), "text_rows": int(tp.shape[0]),
           "speech_row_fraction": xp.shape[0] / (B * N), "text_row_fraction": tp.shape[0] / (B * T)}
    with torch.no_grad():
        # (--only: the other conditionings are not even prepared, so a profile holds one variant's kernels — and one text
        # precompute, counted in the split as well)
        cond_p = eng.prepare_text_packed(tp, ct) if args.only != "varlen" else None
        cond_v = eng.prepare_text(text, N, text_lengths=TL) if args.only != "packed" else None
        cond_d = eng.prepare_text(text, N) if not args.only else None
        sl = torch.tensor(SL, dtype=torch.int32, device="cuda")
        out_p = torch.empty_like(xp)
        fa = lambda: eng.forward_packed(xp, cond_p, t, cu, out=out_p)   # noqa: E731
        fb = lambda: eng.forward(x, cond_v, t, speech_lengths=sl)        # noqa: E731
        fc = lambda: eng.forward(x, cond_d, t)                           # noqa: E731
        if args.only:
            timed(fa if args.only == "packed" else fb, args.steps, 0)
            print(json.dumps({"only": args.only, "steps": args.steps}))
            return
        runs = {"a_packed_ms": [], "b_varlen_ms": [], "c_dense_ms": []}
        for _ in range(args.rounds):
            for k, fn in (("a_packed_ms", fa), ("b_varlen_ms", fb), ("c_dense_ms", fc)):
                runs[k].append(timed(fn, args.steps, args.warmup))
        for k, v in runs.items():
            res[k] = statistics.median(v)
            res[k + "_all"] = v
        res["forward_ratio_a_over_b"] = res["a_packed_ms"] / res["b_varlen_ms"]

        sg = SpeechGenerator(ditto_model=m, device="cuda")
        G, S = 5.0, args.n_steps
        null = torch.zeros(1, T, cfg.text_dim, device="cuda")
        seeds = torch.arange(B, device="cuda") + 1000
        kw = dict(n_steps=S, eta=1.0, guidance=G, seeds=seeds)
        nullp = torch.zeros(1, cfg.text_dim, device="cuda")
        fd = lambda: sg.sample_guided_packed(tp, ct, xp, cu, null_text_emb=nullp, **kw)                     # noqa: E731
        fe = lambda: sg.sample_guided(text, x, speech_lengths=SL, text_lengths=TL, null_text_emb=null, **kw)  # noqa: E731
        gr = {"d_guided_packed_ms_per_step": [], "e_guided_varlen_ms_per_step": []}
        for _ in range(args.guided_rounds):
            for k, fn in (("d_guided_packed_ms_per_step", fd), ("e_guided_varlen_ms_per_step", fe)):
                gr[k].append(timed(fn, 1, 1) / S)
        for k, v in gr.items():
            res[k] = statistics.median(v)
            res[k + "_all"] = v
        res["guided_ratio_d_over_e"] = res["d_guided_packed_ms_per_step"] / res["e_guided_varlen_ms_per_step"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
