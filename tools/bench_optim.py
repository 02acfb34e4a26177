#!/usr/bin/env python3
"""The optimizer tail of a training step on the C2 parameter set (12 layers, d = 768; every parameter that gets a gradient, synthetic
gradients of a fixed seed), in ONE process, the arms alternating round by round:
  (a) torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.AdamW(fused=True) + torch._foreach_lerp_ (the EMA)
  (b) ditto_tts_amd.optim.AdamW with max_norm and ema_decay          (norm partial, norm finish, apply: three launches)
  (c) torch.optim.AdamW(fused=True) alone
  (d) ditto_tts_amd.optim.AdamW with clipping and the EMA off        (one launch)
Every arm owns clones of the parameters and its own state; (a) also owns its gradients (clip_grad_norm_ scales them in place).  ms per
step from device events around --steps steps, --rounds rounds: median, min and max per arm.  The condition recorded: (b) is not
slower than (a) by more than (a)'s own round-to-round range.  Then the launches alone through the C entries (events around
--kernel-iters calls): the two norm launches together, the apply launch with and without the average, the swap — µs and the bytes
each moves per second (4 / 36 / 28 / 16 B per element).  The working set of a step (20 B per parameter, ~2.7 GB here) is ten times
the 256 MB Infinity Cache, but consecutive launches of one step meet what the launch before left there, so the rates are effective
rates of this loop, not HBM rates.  Prints one JSON line and writes it to --out (default profiles/optim_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from ditto_tts_amd import hip, optim
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.synth import synthetic_state_dict

    assert torch.cuda.is_available(), "bench_optim.py measures on the GPU; there is no other path"
    dev = "cuda:0"
    cfg = PRESETS[args.config]["cfg"]
    model = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
    model.load_state_dict(synthetic_state_dict(cfg, seed=1))
    base = [p.detach().to(dev) for n, p in model.named_parameters() if not n.startswith("nac.") and ".attn.out_proj." not in n]
    gen = torch.Generator(device=dev).manual_seed(5)
    grads = [1e-3 * torch.randn(p.shape, generator=gen, device=dev) for p in base]
    n_el = sum(p.numel() for p in base)
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    max_norm, decay, lr, wd = 0.5 * norm, 0.9999, 1e-4, 1e-2

    def clones(own_grads=False):
        ps = [torch.nn.Parameter(p.clone()) for p in base]
        for p, g in zip(ps, grads):
            p.grad = g.clone() if own_grads else g
        return ps

    pa, pb, pc, pd = clones(True), clones(), clones(), clones()
    oa = torch.optim.AdamW(pa, lr=lr, weight_decay=wd, fused=True)
    ea = [p.detach().clone() for p in pa]
    ob = optim.AdamW(pb, lr=lr, weight_decay=wd, max_norm=max_norm, ema_decay=decay)
    oc = torch.optim.AdamW(pc, lr=lr, weight_decay=wd, fused=True)
    od = optim.AdamW(pd, lr=lr, weight_decay=wd)

    def arm_a():
        torch.nn.utils.clip_grad_norm_(pa, max_norm, foreach=True)
        oa.step()
        with torch.no_grad():
            torch._foreach_lerp_(ea, [p.detach() for p in pa], 1.0 - decay)

    arms = [("a_clip_fused_adamw_lerp", arm_a), ("b_fused_clip_ema", ob.step), ("c_fused_adamw", oc.step), ("d_fused_plain", od.step)]

    def timed(fn, steps, warmup=2):
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

    runs = {k: [] for k, _ in arms}
    for r in range(args.rounds):
        order = arms[r % len(arms):] + arms[:r % len(arms)]          # the order rotates round by round
        for k, fn in order:
            runs[k].append(timed(fn, args.steps))
    res = {"config": args.config, "segments": len(base), "parameters": n_el, "steps_per_round": args.steps, "rounds": args.rounds,
           "grad_norm": norm, "max_norm": max_norm, "chunks": sum(hip.optim_chunks(p.numel()) for p in base), "ms_per_step": {}}
    for k, v in runs.items():
        res["ms_per_step"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
    ms = res["ms_per_step"]
    a_range = ms["a_clip_fused_adamw_lerp"]["max"] - ms["a_clip_fused_adamw_lerp"]["min"]
    res["b_minus_a_ms"] = ms["b_fused_clip_ema"]["median"] - ms["a_clip_fused_adamw_lerp"]["median"]
    res["a_round_to_round_range_ms"] = a_range
    res["b_not_slower_than_a_by_more_than_a_range"] = bool(res["b_minus_a_ms"] <= a_range)
    res["d_minus_c_ms"] = ms["d_fused_plain"]["median"] - ms["c_fused_adamw"]["median"]

    # the launches alone, on arm (b)'s tensors and state through the C entries
    st = [ob.state[p] for p in pb]
    rows = np.zeros(len(pb), dtype=optim.SEG_DTYPE)
    ptr = lambda ts: [t.data_ptr() for t in ts]                      # noqa: E731
    sizes = [p.numel() for p in pb]

    def table(with_ema):
        n_chunks = optim.fill_table(rows, (ptr(pb), ptr(grads), ptr([s["exp_avg"] for s in st]), ptr([s["exp_avg_sq"] for s in st]),
                                           ptr([s["ema"] for s in st]) if with_ema else [0] * len(pb)), sizes, [lr] * len(pb),
                                    [wd] * len(pb))
        return torch.from_numpy(rows.view(np.uint8).copy()).to(dev), n_chunks

    t_ema, n_chunks = table(True)
    t_plain, _ = table(False)
    state = torch.frombuffer(bytearray(optim.state_block(0.9, 0.999, 0)), dtype=torch.uint8).to(dev)
    scratch = torch.empty(hip.lib().ditto_optim_scratch_bytes(n_chunks) // 8, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    h_norm = hip.OptimHyper(0.9, 0.999, 1e-8, max_norm, decay, 0, 0)
    h_off = hip.OptimHyper(0.9, 0.999, 1e-8, 0.0, decay, 0, 0)
    phase = [0]

    def k_norm():
        hip.check(hip.call("ditto_optim_grad_norm", table=t_ema.data_ptr(), n_seg=len(pb), n_chunks=n_chunks, hyper=h_norm,
                           state=state.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel() * 8, grid_limit=0, stream=s))

    def k_apply(tab):
        def run():
            hip.check(hip.call("ditto_optim_adamw_step", table=tab.data_ptr(), n_seg=len(pb), n_chunks=n_chunks, hyper=h_off,
                               state=state.data_ptr(), phase=phase[0] & 1, scratch=None, scratch_bytes=0, grid_limit=0, stream=s))
            phase[0] += 1
        return run

    def k_swap():
        hip.check(hip.call("ditto_optim_swap", table=t_ema.data_ptr(), n_seg=len(pb), n_chunks=n_chunks, grid_limit=0, stream=s))

    res["launches"] = {}
    for name, fn, bpe in (("norm_partial_and_finish", k_norm, 4), ("apply_with_ema", k_apply(t_ema), 36),
                          ("apply_without_ema", k_apply(t_plain), 28), ("swap", k_swap, 16)):
        v = [timed(fn, args.kernel_iters) for _ in range(3)]
        us = statistics.median(v) * 1e3
        res["launches"][name] = {"us": us, "us_all": [x * 1e3 for x in v], "bytes": bpe * n_el,
                                 "effective_TB_per_s": bpe * n_el / (us * 1e-6) / 1e12}
    res["note"] = ("effective rates of a loop whose 2.7 GB working set is ~10x the 256 MB Infinity Cache: not HBM rates; the norm "
                   "figure is both launches together (the finish launch is one workgroup over `chunks` doubles)")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
