#!/usr/bin/env python3
"""Digests of the training step's results through the Python host path, for a bitwise comparison between two commits whose
libditto_hip.so is the same: under fixed seeds, sha256 of eps and of every gradient of
  dense    DiTTO.forward under autograd, train mode (dropout 0.1): B = 2, N = 96, T = 40, d = 256, 5 layers — the backward as one
           call, and in pieces of 2 layers through set_grad_sync;
  packed   DiTTO.train_forward_packed, train mode: SL = [200, 77, 130], TL = [96, 40, 65], d = 256, 3 layers — as one call, and in
           pieces of 1 layer through set_grad_sync;
  padded   DiTTO.train_forward (the padded convenience) on the same lengths.
Prints one line per digest and writes them as one JSON object to --out.  Run it at both commits (one process each, the same GPU)
and compare the files: `python tools/train_host_identity.py --compare a.json b.json` prints the count and the differing names and
exits non-zero when any differs."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b):
    da, db = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    print(f"{len(da)} digests in {a}, {len(db)} in {b}: {len(diff)} differ")
    for k in diff:
        print("  differs:", k)
    return 1 if diff or not da else 0


class Rec:
    def reduce(self, piece): pass
    def finish(self): pass
    def abort(self): pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    import torch
    import torch.nn.functional as F
    from ditto_tts_amd.config import DiTTOConfig
    from ditto_tts_amd.modules import DiTTO
    from ditto_tts_amd.synth import hash_normal, synthetic_inputs, synthetic_state_dict
    out = {}

    def sha(t):
        return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()

    def build(cfg, seed):
        m = DiTTO(cfg.hidden_dim, cfg.num_layers, cfg.num_heads, cfg.time_dim, cfg.text_dim, cfg.diffusion_steps)
        m.load_state_dict(synthetic_state_dict(cfg, seed))
        return m.to("cuda").train()

    def case(name, cfg, sync, per_piece, forward, target):
        m = build(cfg, 17)
        m.set_grad_sync(sync, per_piece)
        torch.manual_seed(1234)
        eps = forward(m)
        F.mse_loss(eps, target).backward()
        out[f"{name}/eps"] = sha(eps)
        for n, p in m.named_parameters():
            if p.grad is not None:
                out[f"{name}/{n}"] = sha(p.grad)

    cfg = DiTTOConfig(256, 5, 4, 64, 256, 20)
    B, N, T = 2, 96, 40
    x, text, t = (z.cuda() for z in synthetic_inputs(cfg, B, N, T, seed=31))
    target = hash_normal((B, N, 256), "noise", 32).cuda()
    case("dense_whole", cfg, None, 1, lambda m: m(x, text, t), target)
    case("dense_pieces_of_2", cfg, Rec(), 2, lambda m: m(x, text, t), target)

    cfg = DiTTOConfig(256, 3, 4, 256, 256, 50)
    SL, TL = [200, 77, 130], [96, 40, 65]
    cu, cu_t = [0, 200, 277, 407], [0, 96, 136, 201]
    xp = hash_normal((cu[-1], 256), "px", 11).cuda()
    tp = hash_normal((cu_t[-1], 256), "ptext", 12).cuda()
    tt = torch.tensor([3, 10, 17]).cuda()
    target_p = hash_normal((cu[-1], 256), "pnoise", 13).cuda()
    case("packed_whole", cfg, None, 1, lambda m: m.train_forward_packed(xp, cu, tp, cu_t, tt), target_p)
    case("packed_grad_sync", cfg, Rec(), 1, lambda m: m.train_forward_packed(xp, cu, tp, cu_t, tt), target_p)
    Np, Tp = 208, 100
    xd, td, tgt = torch.zeros(3, Np, 256, device="cuda"), torch.zeros(3, Tp, 256, device="cuda"), torch.zeros(3, Np, 256, device="cuda")
    for b in range(3):
        xd[b, :SL[b]], tgt[b, :SL[b]] = xp[cu[b]:cu[b + 1]], target_p[cu[b]:cu[b + 1]]
        td[b, :TL[b]] = tp[cu_t[b]:cu_t[b + 1]]
    case("padded_convenience", cfg, None, 1, lambda m: m.train_forward(xd, td, tt, speech_lengths=SL, text_lengths=TL), tgt)

    for k, v in out.items():
        print(v, k)
    print(f"{len(out)} digests")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
