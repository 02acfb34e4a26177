#!/usr/bin/env python3
"""Speech-prompted sampling and the span-masked loss at C2 (synthetic weights, B = 32): the lengths of tools/bench_varlen.py
(random.Random(2026): G_b in [256, 1024], T_b in [64, 1024]) as GENERATED frames, each utterance behind a 150-row prompt.  In ONE
process, alternating round by round (25 steps, guidance 5.0, eta 1, per-utterance seeds):
  (a) sample_guided_packed(prompt_lengths=) per step against (b) the unprompted call on utterances of the same total lengths P + G;
  the update kernel alone, prompted against unprompted, in both forms (scalar tag, per-utterance tags), with its bytes and TB/s
  (20 B per generated element: x, eps_c, eps_u read, both halves written; the Philox draw costs no traffic).
--span-loss: DiTTO.span_loss_packed (seeded: eps read, grad written) forward + backward against F.mse_loss on the generated rows
  gathered by index, on the same packed batch.
Prints one JSON line (and writes it to --out): per quantity the median of --rounds rounds and every round."""
import argparse
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=150)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--span-loss", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
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
    B, P, d = args.batch, args.prompt, cfg.hidden_dim
    rng = random.Random(2026)
    GL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    cu, ct = cumulate([g + P for g in GL]), cumulate(TL)
    S = cu[-1]
    m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1))
    m = m.to("cuda").eval()
    audio = hash_normal((S, d), "bench_prompt_audio", 1).cuda()
    text = hash_normal((ct[-1], cfg.text_dim), "bench_prompt_text", 2).cuda()
    seeds = torch.arange(B, device="cuda") + 1000
    res = {"config": "C2", "B": B, "prompt_rows": P, "generated_lengths": GL, "text_lengths": TL, "rows": S, "generated_rows": sum(GL),
           "rounds": args.rounds, "n_steps": args.n_steps}

    if args.span_loss:
        eps = hash_normal((S, d), "bench_prompt_eps", 3).cuda()
        z = hash_normal((S, d), "bench_prompt_z", 4).cuda()
        gen = torch.cat([torch.arange(cu[b] + P, cu[b + 1]) for b in range(B)]).cuda()
        pl = [P] * B

        def span():
            e = eps.clone().requires_grad_(True)
            m.span_loss_packed(e, cu, pl, seeds=seeds, tag=7).backward()

        def indexed():
            e = eps.clone().requires_grad_(True)
            F.mse_loss(e[gen], z[gen]).backward()

        res.update(rounds((("span_loss_step_ms", span), ("mse_loss_indexed_step_ms", indexed)), 20, 3))
        res["ratio_span_over_indexed"] = res["span_loss_step_ms"] / res["mse_loss_indexed_step_ms"]
        res["note"] = "each step clones eps [S, d] and runs loss + backward to eps.grad; both sides pay the clone"
    else:
        with torch.no_grad():
            sg = SpeechGenerator(ditto_model=m, device="cuda")
            null = torch.zeros(1, cfg.text_dim, device="cuda")
            kw = dict(n_steps=args.n_steps, eta=1.0, guidance=5.0, seeds=seeds, null_text_emb=null)
            fa = lambda: sg.sample_guided_packed(text, ct, audio, cu, prompt_lengths=[P] * B, **kw)      # noqa: E731
            fb = lambda: sg.sample_guided_packed(text, ct, audio, cu, **kw)                              # noqa: E731
            res.update(rounds((("a_prompted_ms_per_step", fa), ("b_unprompted_ms_per_step", fb)), 1, 1, 1.0 / args.n_steps))
            res["step_ratio_a_over_b"] = res["a_prompted_ms_per_step"] / res["b_unprompted_ms_per_step"]
            # the update kernel alone
            lib = hip.lib()
            x2 = torch.cat([audio, audio])
            eps2 = hash_normal((2 * S, d), "bench_prompt_eps2", 5).cuda()
            cud = torch.tensor(cu, dtype=torch.int32, device="cuda")
            pld = torch.full((B,), P, dtype=torch.int32, device="cuda")
            a, ce, cz, w = (torch.full((B,), v, device="cuda") for v in (0.98, -0.05, 0.1, 5.0))
            tags = torch.full((B,), 31, dtype=torch.int32, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            common = (w.data_ptr(), a.data_ptr(), ce.data_ptr(), cz.data_ptr(), cud.data_ptr())
            tail = (B, S, max(GL) + P, d, 1, st)
            head = (x2.data_ptr(), eps2.data_ptr(), None, seeds.data_ptr())
            ks = (("update_prompt_ms", lambda: hip.check(lib.ditto_guided_update_packed_prompt(*head, 31, *common, pld.data_ptr(), *tail))),
                  ("update_plain_ms", lambda: hip.check(lib.ditto_guided_update_packed(*head, 31, *common, *tail))),
                  ("update_tags_prompt_ms",
                   lambda: hip.check(lib.ditto_guided_update_packed_tags_prompt(*head, tags.data_ptr(), *common, pld.data_ptr(), *tail))),
                  ("update_tags_plain_ms", lambda: hip.check(lib.ditto_guided_update_packed_tags(*head, tags.data_ptr(), *common, *tail))))
            res.update(rounds(ks, args.kernel_iters, 5))
            by = {"prompt": 20 * sum(GL) * d, "plain": 20 * S * d}
            res["update_bytes"] = by
            for k, _ in ks:
                res[k.replace("_ms", "_TBps")] = by["prompt" if "prompt" in k else "plain"] / (res[k] * 1e-3) / 1e12
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
