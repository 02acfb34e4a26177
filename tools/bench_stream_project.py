#!/usr/bin/env python3
"""Projected guidance (APG) in a request stream at C2 (synthetic weights, 32 utterances, the length mix of tools/bench_varlen.py:
random.Random(2026), N_b in [256, 1024], T_b in [64, 1024]; 25 steps, guidance 5.0, eta 1, per-utterance seeds): the protocol of
tools/bench_stream_refresh.py.

A steady-state guided "ddim" stream kept at B = 32: the 32 requests stand at staggered steps of their schedules (a tool's liberty:
their step index is set once after admission), and every request that finishes is replaced by one of the same lengths before the next
step.  Three streams, ONE process, warmed up, alternating round by round:
    plain       made without project=True: the code path as it was before the argument existed, the comparison
    project_off made with project=True, no request projected: what the argument costs a stream that does not use it
    project_on  made with project=True, every request projected with eta = 0, beta = -0.5, r = --threshold
A round is --steps stream steps between two HIP events, submissions, admissions (the newcomers' conditioning), regroups and
retirements included.  Reported per stream: the median [min, max] over the rounds of ms per step and of finished utterances per
second, the regroups per step and the entries the steps ran; and the two differences to `plain` in ms per step, beside the closed
call's 406.5 ms against 404.3 ms over 25 steps (profiles/project_bench.json): about 0.09 ms per step.  No pass mark.
Nothing here measures speech quality: the weights are synthetic.
Prints one JSON line and writes it to --out (default profiles/stream_project_bench.json)."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANES = ("plain", "project_off", "project_on")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="stream steps per timed round")
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps of every stream before the first round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=1.0, help="guidance_norm_threshold of the projected requests")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_project_bench.json"))
    args = ap.parse_args()

    import torch
    from ditto_tts_amd import hip
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
    apg = dict(guidance_projection=0.0, guidance_norm_threshold=args.threshold, guidance_momentum=-0.5)
    res = {"config": "C2", "B": B, "speech_lengths": SL, "text_lengths": TL, "n_steps": NS, "guidance": G, "eta": 1.0, "speech_rows": S,
           "text_rows": S_T, "steps_per_round": args.steps, "warmup_steps": args.warmup, "rounds": args.rounds, "lanes": list(LANES),
           "projection": apg, "weights": "synthetic", "trained_model_run": False, "speech_quality_measured": False,
           "closed_call_ms_25_steps": [406.5, 404.3], "closed_call_diff_ms_per_step": (406.5 - 404.3) / 25,
           "measured_on": "one MI355X, one process, the streams alternating round by round"}

    class Lane:
        """one stream kept full: a finished request's lengths come back as a new request"""

        def __init__(self, name):
            self.name, self.seed = name, 0
            self.stream = sg.guided_stream(guided=True, **caps, **({} if name == "plain" else {"project": True}))
            self.kw = apg if name == "project_on" else {}
            self.slot = {}                                            # handle id -> which of the 32 length pairs it has
            for j in range(B):
                self.submit(j)
            self.counts = dict(steps=0, regroups=0, finished=0)
            self.entries = {}
            batch, run, regroup = self.stream.batch, self.stream.batch.step, self.stream.batch.regroup

            def step(a):
                self.counts["steps"] += 1
                call = hip.call

                def logged(entry, **kw):
                    if entry.startswith("ditto_guided_step_packed"):
                        self.entries[entry] = self.entries.get(entry, 0) + 1
                    return call(entry, **kw)

                hip.call = logged
                try:
                    run(a)
                finally:
                    hip.call = call

            def counted_regroup(plan, a):
                self.counts["regroups"] += 1
                regroup(plan, a)

            batch.step, batch.regroup = step, counted_regroup
            self.step()                                               # admits all 32 at step 0 of their schedules ...
            for j, r in enumerate(self.stream._active):               # ... and spreads them over the schedule
                r.i = 1 + (j * (NS - 1)) // B
            self.run(args.warmup)

        def submit(self, j):
            h = self.stream.submit(texts[j], SL[j], seed=self.seed, guidance=G, null_text_emb=nulls[j], n_steps=NS, eta=1.0, **self.kw)
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
        lanes = [Lane(name) for name in LANES]
        runs = {name: [] for name in LANES}
        for _ in range(args.rounds):
            for lane in lanes:
                runs[lane.name].append(lane.timed(args.steps))
        for lane in lanes:
            name = lane.name
            ms = [t / c["steps"] for t, c in runs[name]]
            ups = [1e3 * c["finished"] / t for t, c in runs[name]]
            tot = {key: sum(c[key] for _, c in runs[name]) for key in runs[name][0][1]}
            res[f"{name}_step_ms"] = statistics.median(ms)
            res[f"{name}_step_ms_min_max"] = [min(ms), max(ms)]
            res[f"{name}_step_ms_all"] = ms
            res[f"{name}_utterances_per_s"] = statistics.median(ups)
            res[f"{name}_utterances_per_s_min_max"] = [min(ups), max(ups)]
            res[f"{name}_utterances_per_s_all"] = ups
            res[f"{name}_regroups_per_step"] = tot["regroups"] / tot["steps"]
            res[f"{name}_entries"] = lane.entries
        for name in LANES[1:]:
            res[f"{name}_minus_plain_ms_per_step"] = res[f"{name}_step_ms"] - res["plain_step_ms"]
            res[f"{name}_step_over_plain"] = res[f"{name}_step_ms"] / res["plain_step_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
