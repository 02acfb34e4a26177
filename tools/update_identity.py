#!/usr/bin/env python3
"""The packed update, multistep and span-training entries of this tree's libditto_hip.so against a second library built from the
parent commit (--parent-lib), in ONE process on one GPU: first the bits, then the time.

Bits.  Every entry that runs one of the merged kernels — the six ditto_guided_update_packed*, ditto_multistep_update_packed / _window,
ditto_span_noise_packed / _window and ditto_span_mse_packed / _window (gradient and loss) — and ditto_guided_update_packed_reuse, whose
kernels the fold of the row loops left with another machine code, on fixed hashed inputs at the `small` and
`stride` shapes of tests/test_gpu_window_update.py, with that test's P and Q where the entry takes them: every noise mode x CFG on /
off for the updates (the tag form is the entry's), CFG x one step / per-utterance steps x with / without history for the multistep
update, buffer / seeded for the span entries, every noise mode x STORE / LOAD / LOAD with mirror for the reuse update (x2 and the
direction buffer).  sha256 of every output buffer from both libraries; the listing goes to --out-identity
and the exit status is 1 when any digest differs.

Time (skipped with --no-bench).  tools/bench_window.py's shapes: C2, B = 32, the lengths of tools/bench_varlen.py as generated frames
with a 150-row prefix and suffix around each.  Each entry alone (CFG and Philox noise for the updates, a step with history for the
multistep ones, seeded span entries, the reuse update at every noise mode x STORE / LOAD) from this library, the parent's, and the parent's a second time as the A/A pair, the order of the
three rotating round by round; and the whole sample_guided_packed call (25 steps) the same way, one model alive at a time.  Per arm:
the three medians, merged / parent, and the per-round parent / parent ratios (and their reciprocals) whose range is the spread a
merged / parent ratio has to lie in.  --arms TEXT times only the entries whose name contains TEXT and leaves the whole call out.
One JSON object to --out-bench."""
import argparse
import ctypes as C
import gc
import hashlib
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# tests/test_gpu_window_update.py's SHAPES: d, then (rows, prefix rows, suffix rows) per utterance
SHAPES = {"small": (64, ((5, 0, 0), (1, 0, 0), (9, 8, 0), (7, 3, 3), (6, 0, 4), (12, 2, 3))), "stride": (256, ((4202, 1, 1),))}
# (a, kx, ke, b, g, use_prev): a step with a history, the first step, the last step
WITH, FIRST, LAST = (0.9, 1.2, -0.5, 0.4, -0.15, 1), (0.8, 1.1, -0.45, 0.3, 0.0, 0), (0.0, 1.05, -0.3, 1.0, 0.0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libditto_hip.so built from the parent commit")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--n-steps", type=int, default=25)
    ap.add_argument("--arms", default="", help="time only the entries whose name contains this, and not the whole call")
    ap.add_argument("--out-identity", default=os.path.join(ROOT, "profiles", "update_merge_identity.txt"))
    ap.add_argument("--out-bench", default=os.path.join(ROOT, "profiles", "update_merge_bench.json"))
    args = ap.parse_args()

    import torch
    from ditto_tts_amd import hip
    from ditto_tts_amd.synth import hash_normal

    new = hip.lib()
    old = C.CDLL(os.path.abspath(args.parent_lib))
    for name, (r, a) in hip.SYMBOLS.items():
        getattr(old, name).restype, getattr(old, name).argtypes = r, a
    assert old.ditto_abi_version() == new.ditto_abi_version()
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()                                    # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)                         # noqa: E731

    def cumulate(lens):
        out = [0]
        for n in lens:
            out.append(out[-1] + n)
        return out

    def ok(lib, rc):
        if rc:
            raise RuntimeError(f"rc {rc}: {lib.ditto_last_error().decode(errors='replace')}")

    def coef_table(coefs, w):
        t = torch.zeros(len(coefs), 8, dtype=torch.float32)
        for b, c in enumerate(coefs):
            t[b, :5] = torch.tensor(c[:5])
            t[b, 5] = w[b] if w is not None else 0.0
        t.view(torch.int32)[:, 6] = torch.tensor([int(c[5]) for c in coefs], dtype=torch.int32)
        return t.to(dev)

    def context(kind, P, Q):
        """the context-length arguments of an entry: none, prompt_len, or prompt_len and suffix_len"""
        return {"": (), "_prompt": (ptr(P),), "_window": (ptr(P), ptr(Q))}[kind]

    class Batch:
        """the device buffers of one shape, made once: every call works on clones of x / q and reads the rest"""

        def __init__(self, d, N, P, Q, tag):
            B, S = len(N), sum(N)
            self.d, self.B, self.S, self.max_N = d, B, S, max(N)
            self.cu, self.P, self.Q = i32(cumulate(N)), i32(P), i32(Q)
            self.G = sum(n - p - q for n, p, q in zip(N, P, Q))
            self.x = hash_normal((S, d), tag + "_x", 1).to(dev)
            self.eps = hash_normal((2 * S, d), tag + "_eps", 2).to(dev)
            self.z = hash_normal((S, d), tag + "_z", 3).to(dev)
            self.q = hash_normal((S, d), tag + "_q", 4).to(dev)
            self.delta = hash_normal((S, d), tag + "_delta", 5).to(dev)
            k = torch.arange(B, dtype=torch.float32)
            self.a, self.ce, cz = (0.9 + 0.003 * k).to(dev), (-0.2 + 0.01 * k).to(dev), 0.4 + 0.01 * k
            if B > 3:
                cz[3] = 0.0                                  # a sigma = 0 utterance: the tag form skips its draw
            self.cz, self.w = cz.to(dev), (2.0 + 0.05 * k).to(dev)
            self.ca, self.cs = (0.8 + 0.005 * k).to(dev), (0.6 - 0.005 * k).to(dev)
            self.seeds = (torch.arange(B, dtype=torch.int64) * 2654435761 - 2 ** 33 - 1).to(dev)
            self.tags = i32([(49 + 977 * b) % (1 << 31) for b in range(B)])
            self.partial = torch.zeros(B * 1024, device=dev)
            self.dims = (B, S, self.max_N, d)

        def update(self, lib, tags, kind, noise, cfg, x):
            head = (x.data_ptr(), self.eps.data_ptr(), ptr(self.z) if noise == "buffer" else None,
                    ptr(self.seeds) if noise == "philox" else None, self.tags.data_ptr() if tags else 49, ptr(self.w) if cfg else None,
                    self.a.data_ptr(), self.ce.data_ptr(), self.cz.data_ptr(), self.cu.data_ptr())
            name = "ditto_guided_update_packed" + ("_tags" if tags else "") + kind
            ok(lib, getattr(lib, name)(*head, *context(kind, self.P, self.Q), *self.dims, int(cfg), st))

        def reuse(self, lib, noise, mode, mirror, x, delta):
            """mode 1 STORE (eps [2S, d], delta written), 2 LOAD (eps' first S rows, delta read; mirror: x' to the other half too)"""
            ok(lib, lib.ditto_guided_update_packed_reuse(
                x.data_ptr(), self.eps.data_ptr(), delta.data_ptr(), ptr(self.z) if noise == "buffer" else None,
                ptr(self.seeds) if noise == "philox" else None, 49, self.w.data_ptr(), self.a.data_ptr(), self.ce.data_ptr(),
                self.cz.data_ptr(), self.cu.data_ptr(), self.P.data_ptr(), self.Q.data_ptr(), *self.dims, mode, int(mirror), st))

        def multistep(self, lib, kind, cfg, table, coef, x, q):
            step = None if table is not None else hip.MultistepCoef(*coef[:5], 0.0, int(coef[5]), 0)
            head = (x.data_ptr(), self.eps.data_ptr(), q.data_ptr(), step, ptr(table), ptr(self.w) if cfg and table is None else None,
                    self.cu.data_ptr(), self.P.data_ptr())
            if kind:
                ok(lib, lib.ditto_multistep_update_window(*head, self.Q.data_ptr(), *self.dims, int(cfg), st))
            else:
                ok(lib, lib.ditto_multistep_update_packed(*head, *self.dims, int(cfg), st))

        def span_noise(self, lib, kind, seeded, out):
            zs = (None, self.seeds.data_ptr()) if seeded else (self.z.data_ptr(), None)
            ok(lib, getattr(lib, "ditto_span_noise" + kind)(self.x.data_ptr(), *zs, 7, self.ca.data_ptr(), self.cs.data_ptr(),
                                                          self.cu.data_ptr(), *context("_prompt" if kind == "_packed" else kind, self.P,
                                                                                       self.Q), out.data_ptr(), *self.dims, st))

        def span_mse(self, lib, kind, seeded, grad, loss):
            zs = (None, self.seeds.data_ptr()) if seeded else (self.z.data_ptr(), None)
            ok(lib, getattr(lib, "ditto_span_mse" + kind)(self.eps.data_ptr(), *zs, 7, self.cu.data_ptr(),
                                                        *context("_prompt" if kind == "_packed" else kind, self.P, self.Q),
                                                        self.G * self.d, grad.data_ptr(), loss.data_ptr(), self.partial.data_ptr(),
                                                        self.partial.numel() * 4, *self.dims, st))

    # ------------------------------------------------------------------------------------------------ the bits
    def sha(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()

    def digests(lib):
        out = {}
        for shape, (d, npq) in SHAPES.items():
            N, P, Q = ([v[i] for v in npq] for i in range(3))
            bt = Batch(d, N, P, Q, "ui_" + shape)
            for tags in (False, True):
                for kind in ("", "_prompt", "_window"):
                    for noise in ("none", "buffer", "philox"):
                        for cfg in (False, True):
                            x = torch.cat([bt.x, bt.x]) if cfg else bt.x.clone()
                            bt.update(lib, tags, kind, noise, cfg, x)
                            out[f"{shape}/guided_update_packed{'_tags' if tags else ''}{kind}/{noise}/cfg{int(cfg)}/x2"] = sha(x)
            for noise in ("none", "buffer", "philox"):
                for mode, mirror in ((1, False), (2, False), (2, True)):
                    x, delta = torch.cat([bt.x, bt.x]), bt.delta.clone()
                    bt.reuse(lib, noise, mode, mirror, x, delta)
                    key = f"{shape}/guided_update_packed_reuse/{noise}/{'store' if mode == 1 else 'load'}/mirror{int(mirror)}"
                    out[key + "/x2"], out[key + "/delta"] = sha(x), sha(delta)
            for kind in ("", "_window"):
                for cfg in (False, True):
                    for per_utt in (False, True):
                        for coef in (WITH, FIRST):
                            coefs = [(coef, LAST, WITH, FIRST)[b % 4] for b in range(bt.B)]
                            table = coef_table(coefs, bt.w.tolist() if cfg else None) if per_utt else None
                            x, q = torch.cat([bt.x, bt.x]) if cfg else bt.x.clone(), bt.q.clone()
                            bt.multistep(lib, kind, cfg, table, coef, x, q)
                            key = f"{shape}/multistep_update{kind or '_packed'}/cfg{int(cfg)}/per_utt{int(per_utt)}/prev{coef[5]}"
                            out[key + "/x2"], out[key + "/q"] = sha(x), sha(q)
            for kind in ("_packed", "_window"):
                for seeded in (False, True):
                    x_in, grad, loss = torch.full_like(bt.x, 3.0), torch.full_like(bt.x, 3.0), torch.full((1,), 3.0, device=dev)
                    bt.span_noise(lib, kind, seeded, x_in)
                    bt.span_mse(lib, kind, seeded, grad, loss)
                    key = f"{shape}/span{kind}/{'seeded' if seeded else 'buffer'}"
                    out[key + "/x_in"], out[key + "/grad_eps"], out[key + "/loss"] = sha(x_in), sha(grad), sha(loss)
        return out

    dn, do = digests(new), digests(old)
    assert dn.keys() == do.keys() and len(set(dn.values())) > len(dn) // 4
    diff = [k for k in dn if dn[k] != do[k]]
    lines = [f"# sha256 of every output buffer: this tree's libditto_hip.so | the parent's ({torch.cuda.get_device_name(0)})"]
    lines += [f"{dn[k][:16]} | {do[k][:16]}  {'same' if dn[k] == do[k] else 'DIFFERENT'}  {k}" for k in dn]
    lines.append(f"{len(dn)} digests: {len(diff)} differ")
    print("\n".join(lines[-1:] + [f"  differs: {k}" for k in diff]))
    with open(args.out_identity, "w") as f:
        f.write("\n".join(lines) + "\n")
    if diff or args.no_bench:
        sys.exit(1 if diff else 0)

    # ------------------------------------------------------------------------------------------------ the time
    from ditto_tts_amd.config import PRESETS
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.sampler import SpeechGenerator
    from ditto_tts_amd.synth import synthetic_state_dict

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

    def summary(runs):
        """runs: {"merged" | "parent" | "parent_again": per-round ms}"""
        med = {k: statistics.median(v) for k, v in runs.items()}
        aa = [b / a for a, b in zip(runs["parent"], runs["parent_again"])]
        aa += [1.0 / r for r in aa]
        ratio = med["merged"] / med["parent"]
        return {"median_ms": med, "merged_over_parent": ratio, "parent_again_over_parent": med["parent_again"] / med["parent"],
                "aa_round_ratio_min": min(aa), "aa_round_ratio_max": max(aa), "inside_aa_spread": min(aa) <= ratio <= max(aa),
                "rounds_ms": runs}

    cfg = PRESETS["C2"]["cfg"]
    B, d, K = 32, cfg.hidden_dim, 150
    rng = random.Random(2026)
    GL = [rng.randint(256, 1024) for _ in range(B)]
    TL = [rng.randint(64, 1024) for _ in range(B)]
    bt = Batch(d, [g + 2 * K for g in GL], [K] * B, [K] * B, "ub")
    res = {"config": "C2", "B": B, "generated_lengths": GL, "context_rows": K, "rows": bt.S, "rounds": args.rounds,
           "kernel_iters": args.kernel_iters, "device": torch.cuda.get_device_name(0), "kernels": {}}
    x2, q, loss = torch.cat([bt.x, bt.x]), bt.q.clone(), torch.zeros(1, device=dev)
    out1 = torch.empty_like(bt.x)
    arms = {}
    for tags in (False, True):
        for kind in ("", "_prompt", "_window"):
            arms[f"guided_update_packed{'_tags' if tags else ''}{kind}/philox/cfg"] = (
                lambda lib, tags=tags, kind=kind: bt.update(lib, tags, kind, "philox", True, x2))
    for kind in ("", "_window"):
        arms[f"multistep_update{kind or '_packed'}/cfg/history"] = lambda lib, kind=kind: bt.multistep(lib, kind, True, None, WITH, x2, q)
    for kind in ("_packed", "_window"):
        arms[f"span_noise{kind}/seeded"] = lambda lib, kind=kind: bt.span_noise(lib, kind, True, out1)
        arms[f"span_mse{kind}/seeded"] = lambda lib, kind=kind: bt.span_mse(lib, kind, True, out1, loss)
    delta = bt.delta.clone()
    for noise in ("none", "buffer", "philox"):
        for mode in (1, 2):
            arms[f"guided_update_packed_reuse/{noise}/{'store' if mode == 1 else 'load'}"] = (
                lambda lib, noise=noise, mode=mode: bt.reuse(lib, noise, mode, False, x2, delta))
    arms = {k: v for k, v in arms.items() if args.arms in k}
    trio = [("merged", new), ("parent", old), ("parent_again", old)]
    for name, fn in arms.items():
        runs = {k: [] for k, _ in trio}
        for rnd in range(args.rounds):
            for k, lib in trio[rnd % 3:] + trio[:rnd % 3]:
                runs[k].append(timed(lambda: fn(lib), args.kernel_iters, 10))
        res["kernels"][name] = summary(runs)
        x2.copy_(torch.cat([bt.x, bt.x]))
        q.copy_(bt.q)

    # the whole sample_guided_packed call, one model alive at a time (tools/bench_window.py's arm (c))
    legs = dict(res["kernels"])
    if not args.arms:
        state = synthetic_state_dict(cfg, seed=1)
        cg, ct = cumulate(GL), cumulate(TL)
        audio = hash_normal((cg[-1], d), "bench_window_audio", 1).to(dev)
        text = hash_normal((ct[-1], cfg.text_dim), "bench_window_text", 2).to(dev)
        seeds, null = torch.arange(B, device=dev) + 1000, torch.zeros(1, cfg.text_dim, device=dev)
        runs, outputs = {k: [] for k, _ in trio}, {}
        with torch.no_grad():
            for rnd in range(args.rounds):
                for k, lib in trio[rnd % 3:] + trio[:rnd % 3]:
                    hip._lib = lib
                    try:
                        m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
                        m.load_state_dict(state)
                        g = SpeechGenerator(ditto_model=m.to(dev).eval(), device=dev)
                        assert g.ditto_model.engine(torch.device("cuda:0")).lib is lib
                    finally:
                        hip._lib = new
                    f = lambda: g.sample_guided_packed(text, ct, audio, cg, n_steps=args.n_steps, eta=1.0, seeds=seeds, guidance=5.0,  # noqa: E731
                                                       null_text_emb=null)
                    runs[k].append(timed(f, 1, 1))
                    if rnd == 0:
                        outputs[k] = f().cpu()
                    del g, m, f
                    gc.collect()
                    torch.cuda.empty_cache()
        assert torch.equal(outputs["merged"], outputs["parent"])
        res["sample_guided_packed"] = legs["sample_guided_packed"] = dict(summary(runs), n_steps=args.n_steps, output_equals_parent=True)
    res["outside_aa_spread"] = [k for k, v in legs.items() if not v["inside_aa_spread"]]
    for k, v in legs.items():
        print(f"{v['median_ms']['merged'] * 1e3:10.2f} us merged {v['median_ms']['parent'] * 1e3:10.2f} us parent  ratio "
              f"{v['merged_over_parent']:.4f}  A/A [{v['aa_round_ratio_min']:.4f}, {v['aa_round_ratio_max']:.4f}]  "
              f"{'inside' if v['inside_aa_spread'] else 'OUTSIDE'}  {k}")
    with open(args.out_bench, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
