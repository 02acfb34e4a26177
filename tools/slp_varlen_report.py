"""Timing of the speech-length predictor on variable-length batches on one MI355X.

    python tools/slp_varlen_report.py [--out profiles/FILE.txt]      # one JSON line per configuration

One process, every shape warmed up first, then ROUNDS alternating rounds of
    (a) the dense entry (ditto_slp_forward: the code a call without lengths runs),
    (b) the varlen entry with full lengths, slp_last_row = 1 (last layer on the last rows only),
    (c) the same with slp_last_row = 0 (every layer GEMM-composed),
    (d) a mixed-length batch, lengths uniform in [S/4, S] and [T/4, T] (seeded), slp_last_row = 1,
    (e) the same utterances as one dense call each, on their own slices.
Each figure is the mean of REPS calls between two HIP events; min / median / max are over the rounds.  (a) is the
yardstick: (b) counts as faster only if max(b) < min(a), i.e. by more than (a)'s own spread."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ditto_tts_amd import hip  # noqa: E402
from ditto_tts_amd.slp import SLP  # noqa: E402
from ditto_tts_amd.synth import hash_normal, synthetic_slp_state_dict  # noqa: E402

ROUNDS, REPS = 5, 40


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--T", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slp_varlen_report needs an MI355X: there is no CPU path and nothing to time without one")
    B, S, T, ncls = args.B, args.S, args.T, 11
    lines = []
    for d, nhead, nl in [(1472, 1, 1), (1472, 4, 4)]:         # ConfigSLP; SLP()'s defaults on byt5-small
        m = SLP(ncls, nhead, nl, hidden_size=d)
        m.load_state_dict(synthetic_slp_state_dict(d, nhead, nl, ncls, 3))
        m = m.to("cuda").eval()
        zt, za = hash_normal((B, T, d), "t", 3).cuda(), hash_normal((B, S, d), "a", 3).cuda()
        g = torch.Generator().manual_seed(5)
        alen = torch.randint(S // 4, S + 1, (B,), generator=g).tolist()
        tlen = torch.randint(max(T // 4, 1), T + 1, (B,), generator=g).tolist()
        full_a, full_t = [S] * B, [T] * B
        slices = [(zt[b:b + 1, :tlen[b]].contiguous(), za[b:b + 1, :alen[b]].contiguous()) for b in range(B)]

        def opt(v):
            hip.set_option("slp_last_row", v)

        def a():
            m.decode(zt, za)

        def b():
            m.decode(zt, za, audio_lengths=full_a, text_lengths=full_t)

        def dmix():
            m.decode(zt, za, audio_lengths=alen, text_lengths=tlen)

        def e():
            for t_, a_ in slices:
                m.decode(t_, a_)
        runs = [("a_dense", a, 1), ("b_varlen_full_last_row", b, 1), ("c_varlen_full_composed", b, 0),
                ("d_mixed_batch", dmix, 1), ("e_mixed_one_call_each", e, 1)]
        try:
            for _, fn, v in runs:                               # warm-up of every shape and path
                opt(v)
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k, _, _ in runs}
            for _ in range(ROUNDS):                             # alternating rounds
                for k, fn, v in runs:
                    opt(v)
                    ms[k].append(timed(fn))
        finally:
            opt(1)
        rec = {"d_model": d, "nhead": nhead, "layers": nl, "B": B, "S": S, "T": T, "rounds": ROUNDS, "reps": REPS,
               "lr_chunk": hip.get_option("slp_lr_chunk"), "audio_lengths": alen, "text_lengths": tlen,
               "ms": {k: stats(v) for k, v in ms.items()}}
        rec["b_faster_than_a_beyond_spread"] = max(ms["b_varlen_full_last_row"]) < min(ms["a_dense"])
        rec["d_faster_than_e"] = max(ms["d_mixed_batch"]) < min(ms["e_mixed_one_call_each"])
        rec["a_over_b_median"] = round(statistics.median(ms["a_dense"]) / statistics.median(ms["b_varlen_full_last_row"]), 3)
        rec["e_over_d_median"] = round(statistics.median(ms["e_mixed_one_call_each"]) / statistics.median(ms["d_mixed_batch"]), 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del m
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
