#!/usr/bin/env python3
"""Digests of the guided sampling calls through the public Python API, for a bitwise comparison between two commits whose kernels
are the same and whose host path above them is not: under fixed seeds, at DiTTOConfig(256, 2, 4, 256, 256, 50) and the shapes of
tests/test_gpu_refresh_sampler.py (lengths 96, 50, 70; texts 40, 7, 19; 6 steps), sha256 of
  packed   sample_guided_packed for solver "ddim" and "dpmpp2m" x {no guidance, guidance, interval (10, 35), rescale 0.7, prompts,
           prompts + suffixes, guidance_refresh=2 alone and with the interval, prediction="v", batch_class=3}; DDIM also at eta = 1
           with seeds=, with noises= and with torch.manual_seed and neither;
  padded   sample_guided with and without guidance and lengths;
  stream   one guided_stream drain per solver over five requests that differ in steps, interval, phi and prompt (the tags, mixed,
           per-utterance-coefficient and rescale entries all run), and one infill stream.
Prints one line per digest and writes them as one JSON object to --out.  Run it at both commits (one process each, the same GPU)
and compare: `python tools/step_host_identity.py --compare a.json b.json` prints the count and the differing names and exits non-zero
when any differs.

Host time: `--time` prints one JSON line with the time of the 25-step sample_guided_packed call at the shapes of
tools/bench_refresh.py (C2, B = 32; guided DDIM, guided 2M, DDIM with guidance_refresh=2), one warm-up and --iters timed calls each,
in this process.  `--bench PARENT_ROOT` runs that in fresh processes — this tree, the parent's checkout and the parent's again as the
A/A pair, the order rotating over --rounds — and writes medians, tree / parent and the range of the per-round parent / parent ratios
to --out."""
import argparse
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(a, b):
    da, db = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    print(f"{len(da)} digests in {a}, {len(db)} in {b}: {len(diff)} differ")
    for k in diff:
        print("  differs:", k)
    return 1 if diff or not da else 0


def cumulate(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def generator(cfg, seed):
    import torch
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator
    from ditto_tts_amd.synth import synthetic_state_dict
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed))
    return SpeechGenerator(ditto_model=m.to("cuda").eval(), device="cuda"), torch


def digests(out_path):
    from ditto_tts_amd.config import DiTTOConfig
    from ditto_tts_amd.synth import hash_normal
    cfg = DiTTOConfig(256, 2, 4, 256, 256, 50)
    sg, torch = generator(cfg, 3)
    out = {}

    def sha(t):
        return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()

    LENS, TEXTS, T_NULL, NS, B = (96, 50, 70), (40, 7, 19), 16, 6, 3
    cu, ct, cn = cumulate(LENS), cumulate(TEXTS), cumulate([T_NULL] * B)
    S, D = cu[-1], cfg.hidden_dim
    text = hash_normal((ct[-1], cfg.text_dim), "sh_text", 1).cuda()
    null = hash_normal((cn[-1], cfg.text_dim), "sh_null", 2).cuda()
    start = hash_normal((S, D), "sh_start", 3).cuda()
    guided = dict(guidance=[3.0, 2.0, 4.5], null_text_emb=null, null_text_cu_seqlens=cn)
    prompts, suffixes = (20, 0, 9), (0, 11, 5)
    variants = {"unguided": {}, "guided": guided, "interval": dict(guided, guidance_interval=(10, 35)),
                "rescale": dict(guided, guidance_rescale=0.7), "prompts": dict(guided, prompt_lengths=prompts),
                "prompts_suffixes": dict(guided, prompt_lengths=prompts, suffix_lengths=suffixes),
                "refresh2": dict(guided, guidance_refresh=2), "refresh2_interval": dict(guided, guidance_refresh=2, guidance_interval=(10, 35)),
                "v": dict(guided, prediction="v"), "batch_class3": dict(guided, batch_class=3)}
    with torch.no_grad():
        for solver in ("ddim", "dpmpp2m"):
            for name, kw in variants.items():
                x = sg.sample_guided_packed(text, ct, start, cu, n_steps=NS, eta=0.0, seeds=torch.tensor([21, 22, 23]),
                                            cond_by_audio=True, solver=solver, **kw)
                out[f"packed/{solver}/{name}"] = sha(x)
        noises = [hash_normal((S, D), "sh_noise", i).cuda() for i in range(NS)]
        for name, kw in (("seeds", dict(seeds=torch.tensor([21, 22, 23]), cond_by_audio=True)), ("noises", dict(noises=noises, cond_by_audio=True)),
                         ("manual_seed", dict(cond_by_audio=True)), ("manual_seed_x_T_drawn", {})):
            torch.manual_seed(1234)
            x = sg.sample_guided_packed(text, ct, start, cu, n_steps=NS, eta=1.0, **guided, **kw)
            out[f"packed/ddim/eta1_{name}"] = sha(x)
            out[f"packed/ddim/eta1_{name}/generator_after"] = sha(torch.rand(4, device="cuda"))

        N, T = 64, 24
        xp = hash_normal((B, N, D), "sh_padded", 4).cuda()
        tp = hash_normal((B, T, cfg.text_dim), "sh_ptext", 5).cuda()
        np_ = hash_normal((1, T, cfg.text_dim), "sh_pnull", 6).cuda()
        lens = dict(speech_lengths=[64, 33, 50], text_lengths=[24, 7, 19])
        for name, kw in (("unguided", {}), ("guided", dict(guidance=2.5, null_text_emb=np_)), ("unguided_lengths", lens),
                         ("guided_lengths", dict(lens, guidance=[3.0, 2.0, 4.5], null_text_emb=np_))):
            x = sg.sample_guided(tp, xp, n_steps=NS, eta=1.0, seeds=torch.tensor([31, 32, 33]), cond_by_audio=True, **kw)
            out[f"padded/{name}"] = sha(x)

        caps = dict(max_rows=512, max_utterances=3, max_text_rows=256)
        texts = [hash_normal((t, cfg.text_dim), "sh_stext", k) for k, t in enumerate((40, 7, 19, 30, 12))]
        nulls = [hash_normal((T_NULL + k, cfg.text_dim), "sh_snull", k) for k in range(5)]
        prompt = hash_normal((20, D), "sh_sprompt", 1)
        suffix = hash_normal((11, D), "sh_ssuffix", 2)
        # (frames, steps, per-request arguments): steps, interval, phi and prompt all differ; the fourth and fifth wait for room
        reqs = [(96, 6, {}), (50, 4, dict(guidance_interval=(10, 35))), (70, 5, dict(guidance_rescale=0.7, prompt=prompt)),
                (60, 6, dict(guidance_interval=(20, 49), guidance_rescale=0.3)), (33, 3, dict(prompt=prompt))]
        for solver in ("ddim", "dpmpp2m"):
            stream = sg.guided_stream(guided=True, solver=solver, **caps)
            ids = {}
            for k, (frames, steps, kw) in enumerate(reqs):
                if solver != "ddim":                                               # a 2M stream serves no intervals
                    kw = {a: v for a, v in kw.items() if a != "guidance_interval"}
                h = stream.submit(texts[k], frames, seed=500 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps,
                                  eta=1.0 if solver == "ddim" else 0.0, **kw)
                ids[h.id] = k
            for h, x in stream.drain():
                out[f"stream/{solver}/request{ids[h.id]}"] = sha(x)
        stream = sg.guided_stream(guided=True, infill=True, **caps)
        ids = {}
        for k, (frames, steps, kw) in enumerate([(96, 6, dict(suffix=suffix)), (50, 4, dict(prompt=prompt, suffix=suffix)), (70, 5, {})]):
            ids[stream.submit(texts[k], frames, seed=600 + k, guidance=2.0 + k, null_text_emb=nulls[k], n_steps=steps, eta=1.0, **kw).id] = k
        for h, x in stream.drain():
            out[f"stream/infill/request{ids[h.id]}"] = sha(x)

    for k, v in out.items():
        print(v, k)
    print(f"{len(out)} digests")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=0, sort_keys=True)


def time_calls(iters):
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.synth import hash_normal
    cfg = PRESETS["C2"]["cfg"]
    sg, torch = generator(cfg, 1)
    B, d = 32, cfg.hidden_dim
    rng = random.Random(2026)
    NL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    cu, ct = cumulate(NL), cumulate(TL)
    audio = hash_normal((cu[-1], d), "bench_refresh_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_refresh_text", 2).cuda()
    seeds, null = torch.arange(B, device="cuda") + 1000, torch.zeros(1, cfg.text_dim, device="cuda")
    res = {}
    with torch.no_grad():
        for name, kw in (("ddim", dict(eta=1.0)), ("dpmpp2m", dict(solver="dpmpp2m")), ("ddim_refresh2", dict(eta=1.0, guidance_refresh=2))):
            f = lambda: sg.sample_guided_packed(text, ct, audio, cu, n_steps=25, seeds=seeds, guidance=5.0, null_text_emb=null, **kw)  # noqa: E731
            f()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize()
            res[name] = a.elapsed_time(b) / iters
    print("TIME " + json.dumps(res), flush=True)


def bench(parent_root, rounds, iters, out_path):
    trio = [("tree", ROOT), ("parent", parent_root), ("parent_again", parent_root)]
    runs = {}
    for rnd in range(rounds):
        for arm, root in trio[rnd % 3:] + trio[:rnd % 3]:
            p = subprocess.run([sys.executable, os.path.join(root, "tools", "step_host_identity.py"), "--time", "--iters", str(iters)],
                               capture_output=True, text=True, cwd=root, timeout=300)
            if p.returncode:
                sys.exit(f"{arm} failed with {p.returncode}:\n{p.stdout}\n{p.stderr}")    # nothing more is started on the GPU
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("TIME ")][-1]
            for k, ms in json.loads(line[5:]).items():
                runs.setdefault(k, {}).setdefault(arm, []).append(ms)
            print(rnd, arm, line, flush=True)
    res = {"config": "C2", "B": 32, "n_steps": 25, "rounds": rounds, "iters": iters, "one_process_per_arm_and_round": True, "calls": {}}
    for k, r in runs.items():
        med = {arm: statistics.median(v) for arm, v in r.items()}
        aa = [b / a for a, b in zip(r["parent"], r["parent_again"])]
        aa += [1.0 / x for x in aa]
        ratio = med["tree"] / med["parent"]
        res["calls"][k] = {"median_ms": med, "tree_over_parent": ratio, "parent_again_over_parent": med["parent_again"] / med["parent"],
                           "aa_round_ratio_min": min(aa), "aa_round_ratio_max": max(aa), "inside_aa_spread": min(aa) <= ratio <= max(aa),
                           "rounds_ms": r}
        print(f"{k}: tree {med['tree']:.2f} ms, parent {med['parent']:.2f} ms, ratio {ratio:.4f}, A/A [{min(aa):.4f}, {max(aa):.4f}]")
    with open(out_path, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--bench", metavar="PARENT_ROOT")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.time:
        return time_calls(args.iters)
    if args.bench:
        return bench(os.path.abspath(args.bench), args.rounds, args.iters,
                     args.out or os.path.join(ROOT, "profiles", "step_host_identity_bench.json"))
    digests(args.out)


if __name__ == "__main__":
    main()
