"""In-process A/B of the per-clip step against the universal step (run on the GPU box): replayed hipGraphs of one PGD step at
32 x 10 s, base architecture, fp32-parity, snr 40, alternating rounds on one device —

    universal   PgdStepper, p (1, L), the gradient summed over the 32 clips
    per-clip    ClipStepper, delta (32, L), one gradient row and one projection per clip
    32 x B=1    the per-clip mode's real competitor: 32 sequential batch-1 universal steps over the same clips (one graph on a
                fixed one-clip buffer; the clip and its perturbation row are copied in and out around each replay)

Prints ms/step per variant (median, min and max over the rounds) and the per-clip / universal ratio.

    python tools/clip_step_ab.py [--steps 10] [--rounds 5]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from paa_amd import arch as A, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils import parser
from paa_amd.training_utils.clip_attack import ClipStepper
from paa_amd.training_utils.pgd import PgdStepper


def _time(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    o = ap.parse_args()
    a, B, L = A.BASE, o.batch, int(o.seconds * 16000)
    args = parser.create_arg_parser().parse_args(["--norm_type", "snr", "--snr_db", "40", "--lr", "1e-4", "--optimizer_type", "pgd",
                                                  "--device", "cuda", "--dtype", o.dtype])
    texts = [("the quick brown fox jumps over a lazy dog and runs " * 4)[:150] for _ in range(B)]
    labels = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, o.dtype)
    p = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
    delta = p.repeat(B, 1).contiguous()
    uni = PgdStepper(m, args, L)
    g_uni, _ = uni.capture(p, clean, labels)
    clip = ClipStepper(m, args, L)
    g_clip, _ = clip.capture(delta, clean, labels)
    one = PgdStepper(m, args, L)
    clean1, p1, lab1 = clean[:1].clone(), p.clone().view(1, L), labels[:1].clone()
    g_one, _ = one.capture(p1, clean1, lab1)
    rows = p.repeat(B, 1).contiguous()

    def seq():
        for b in range(B):
            clean1.copy_(clean[b:b + 1])
            lab1.copy_(labels[b:b + 1])
            p1.copy_(rows[b:b + 1])
            g_one.replay()
            rows[b:b + 1].copy_(p1)

    variants = {"universal": g_uni.replay, "per-clip": g_clip.replay, f"{B} x B=1": seq}
    res = {k: [] for k in variants}
    for rnd in range(o.rounds + 1):
        for k, fn in variants.items():
            ms = _time(fn, o.steps if k != f"{B} x B=1" else max(1, o.steps // 3))
            if rnd:                                          # round 0 is the warm-up
                res[k].append(ms)
    print(f"{B} x {o.seconds:g} s, base, {o.dtype}, snr 40, replayed graphs, {o.rounds} rounds of {o.steps} steps:")
    for k, v in res.items():
        v = np.array(v)
        print(f"  {k:12s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  spread {100 * (v.max() - v.min()) / np.median(v):.1f} %")
    ratio = np.median(res["per-clip"]) / np.median(res["universal"])
    print(f"  per-clip / universal = {ratio:.4f};  {B} x B=1 / per-clip = {np.median(res[f'{B} x B=1']) / np.median(res['per-clip']):.2f}")
    assert torch.isfinite(delta).all() and torch.isfinite(p).all()


if __name__ == "__main__":
    main()
