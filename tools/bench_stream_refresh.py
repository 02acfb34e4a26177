#!/usr/bin/env python3
"""Guidance reuse in a request stream at C2 (synthetic weights, 32 utterances, the length mix of tools/bench_varlen.py:
random.Random(2026), N_b in [256, 1024], T_b in [64, 1024]; 25 steps, guidance 5.0, eta 1, per-utterance seeds).

A steady-state guided "ddim" stream made with refresh=True and kept at B = 32: the 32 requests stand at staggered steps of their
schedules (a tool's liberty: their step index is set once after admission), every request that finishes is replaced by one of the same
lengths before the next step, and every request of a stream has the same guidance_refresh = k.  One stream per k in --ks (default 1, 2,
3, 5), ONE process, warmed up, the streams alternating round by round; a round is --steps stream steps between two HIP events,
submissions, admissions (the newcomers' conditioning), regroups and retirements included.  Reported per k: the median [min, max] over
the rounds of ms per step and of finished utterances per second, the mean rows of the forward (S + S_G), the mean size of the
refreshing set and the regroups per step.  k = 1 in the same run is the comparison: the code path of a stream without the argument,
on the same box.  The expectation to check against is forward rows of about S (1 + 1 / k) instead of 2 S.
Nothing here measures speech quality: the weights are synthetic.
Prints one JSON line and writes it to --out (default profiles/stream_refresh_bench.json)."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="stream steps per timed round")
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps of every stream before the first round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 3, 5])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_refresh_bench.json"))
    args = ap.parse_args()

    import torch
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator
    from ditto_tts_amd.synth import hash_normal, synthetic_state_dict

    cfg = PRESETS["C2"]["cfg"]
    B, G, NS = args.batch, 5.0, args.n_steps
    rng = random.Random(2026)
    SL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    dt = cfg.text_dim
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").eval()
    sg = SpeechGenerator(ditto_model=m, device="cuda")
    texts = [hash_normal((t, dt), "bench_text", k).cuda() for k, t in enumerate(TL)]
    nulls = [torch.zeros(t, dt, device="cuda") for t in TL]
    S, S_T = sum(SL), sum(TL)
    caps = dict(max_rows=S, max_utterances=B, max_text_rows=2 * S_T)
    res = {"config": "C2", "B": B, "speech_lengths": SL, "text_lengths": TL, "n_steps": NS, "guidance": G, "eta": 1.0, "speech_rows": S,
           "text_rows": S_T, "steps_per_round": args.steps, "warmup_steps": args.warmup, "rounds": args.rounds, "ks": args.ks,
           "weights": "synthetic", "trained_model_run": False, "speech_quality_measured": False,
           "measured_on": "one MI355X, one process, the streams alternating round by round"}

    class Lane:
        """one stream with every request at refresh period k, kept full: a finished request's lengths come back as a new request"""

        def __init__(self, k):
            self.k, self.seed = k, 0
            self.stream = sg.guided_stream(guided=True, refresh=True, **caps)
            self.slot = {}                                            # handle id -> which of the 32 length pairs it has
            for j in range(B):
                self.submit(j)
            self.counts = dict(steps=0, rows=0, G=0, regroups=0, finished=0)
            batch, run, regroup = self.stream.batch, self.stream.batch.step, self.stream.batch.regroup

            def step(a):
                c = self.counts
                c["steps"], c["rows"], c["G"] = c["steps"] + 1, c["rows"] + a.S + a.S_G, c["G"] + a.G
                run(a)

            def counted_regroup(plan, a):
                self.counts["regroups"] += 1
                regroup(plan, a)

            batch.step, batch.regroup = step, counted_regroup
            self.step()                                               # admits all 32 at step 0 of their schedules ...
            for j, r in enumerate(self.stream._active):               # ... and spreads them over the schedule
                r.i = 1 + (j * (NS - 1)) // B
            self.run(args.warmup)

        def submit(self, j):
            h = self.stream.submit(texts[j], SL[j], seed=1000 * self.k + self.seed, guidance=G, null_text_emb=nulls[j], n_steps=NS, eta=1.0,
                                   guidance_refresh=self.k)
            self.slot[h.id] = j
            self.seed += 1

        def step(self):
            for h, _ in self.stream.step():
                self.counts["finished"] += 1
                self.submit(self.slot.pop(h.id))

        def run(self, steps):
            for _ in range(steps):
                self.step()

        def timed(self, steps):
            before = dict(self.counts)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.run(steps)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            return ms, {key: self.counts[key] - before[key] for key in before}

    with torch.no_grad():
        lanes = [Lane(k) for k in args.ks]
        runs = {k: [] for k in args.ks}
        for _ in range(args.rounds):
            for lane in lanes:
                runs[lane.k].append(lane.timed(args.steps))
        for k in args.ks:
            ms = [t / c["steps"] for t, c in runs[k]]
            ups = [1e3 * c["finished"] / t for t, c in runs[k]]
            tot = {key: sum(c[key] for _, c in runs[k]) for key in runs[k][0][1]}
            res[f"k{k}_step_ms"] = statistics.median(ms)
            res[f"k{k}_step_ms_min_max"] = [min(ms), max(ms)]
            res[f"k{k}_step_ms_all"] = ms
            res[f"k{k}_utterances_per_s"] = statistics.median(ups)
            res[f"k{k}_utterances_per_s_min_max"] = [min(ups), max(ups)]
            res[f"k{k}_utterances_per_s_all"] = ups
            res[f"k{k}_forward_rows_mean"] = tot["rows"] / tot["steps"]
            res[f"k{k}_forward_rows_over_2S"] = tot["rows"] / tot["steps"] / (2 * S)
            res[f"k{k}_row_model_1_plus_1_over_k_over_2"] = (1 + 1 / k) / 2
            res[f"k{k}_refreshing_mean"] = tot["G"] / tot["steps"]
            res[f"k{k}_regroups_per_step"] = tot["regroups"] / tot["steps"]
        if 1 in args.ks:
            for k in args.ks:
                res[f"k{k}_step_over_k1"] = res[f"k{k}_step_ms"] / res["k1_step_ms"]
                res[f"k{k}_utterances_over_k1"] = res[f"k{k}_utterances_per_s"] / res["k1_utterances_per_s"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
