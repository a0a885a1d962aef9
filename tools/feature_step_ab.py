"""Cost of the feature-distance loss on the device steps (run on the GPU box).

The 32 x 10 s base step, untargeted, with --norm_type linf as replayed hipGraphs, alternating in one process, for the universal step
(PgdStepper) and for the per-clip step (ClipStepper):
  ctc, ctc (again)   --loss_type ctc, taken twice: the tool's own run-to-run spread
  feature            --loss_type feature (universal: paa_model_features(clean) inside the graph, then the step with paa_feature_cos in
                     place of CTC and no lm_head input-gradient product; per clip: the reference is computed once, outside the graph)
ms / step (median over all timed steps), spread, and the feature / ctc ratio.  Every replay is synchronised and timed on its own,
and a step that takes longer than --step_limit seconds ends the run (nothing more is launched after it).

    python tools/feature_step_ab.py [--steps 10] [--rounds 5] [--dtype fp32] [--out profiles/feature_step_ab.txt]

After the step legs, paa_feature_cos alone (loss, d and the cotangent) on random rows at 32 x 499 x 768 and 32 x 499 x 1024 in the
model's padded layout: HIP events around 20 calls, median of 5 rounds, with the bytes it moves (2 M H 4 read, M H 4 written) over
that time.  --no_kernels skips this part.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from paa_amd import _lib, arch as A, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils import parser
from paa_amd.training_utils.clip_attack import ClipStepper
from paa_amd.training_utils.pgd import PgdStepper


def _args(dtype, loss_type):
    return parser.create_arg_parser().parse_args(
        ["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda", "--dtype", dtype, "--linf_size", "0.01",
         "--loss_type", loss_type])


def _timed(fn, steps, limit):
    """ms of each of ``steps`` calls, every one synchronised; a call over ``limit`` seconds ends the run."""
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt > limit:
            raise SystemExit(f"a step took {dt:.1f} s (limit {limit:g} s): stopping")
        out.append(dt * 1e3)
    return out


def step_ab(o, say, kind):
    a, B, L = A.BASE, o.batch, int(o.seconds * 16000)
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, o.dtype)
    legs = {"ctc": "ctc", "ctc (again)": "ctc", "feature": "feature"}
    # every leg keeps its own stepper, perturbation and labels alive for as long as its graph is replayed (the graphs hold raw
    # pointers); a graph keeps the loss it was captured with, whatever the model's switch says at replay time
    graphs, deltas, steppers, labels, losses = {}, {}, {}, {}, {}
    for key, lt in legs.items():
        args = _args(o.dtype, lt)
        labels[key] = loss_helpers.make_labels(["the quick brown fox jumps over the lazy dog"] * B, None, args, B).to(device="cuda", dtype=torch.int32)
        if kind == "universal":
            deltas[key] = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
            steppers[key] = PgdStepper(m, args, L)
        else:
            rows = np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * np.float32(2e-3)
            deltas[key] = torch.from_numpy(rows).cuda()
            steppers[key] = ClipStepper(m, args, L)
            if lt == "feature":
                steppers[key].feature_reset(clean)
        graphs[key], r = steppers[key].capture(deltas[key], clean, labels[key])
        losses[key] = r["loss"]
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            ms = _timed(g.replay, o.steps, o.step_limit)
            if rnd:
                res[k] += ms
    say(f"{kind} step, {B} x {o.seconds:g} s, base, {o.dtype}, linf, untargeted ({labels['ctc'].shape[1]} label slots, "
        f"{m.frames} frames), replayed graphs, {o.rounds} rounds of {o.steps} steps, alternating, every step synchronised:")
    for k, v in res.items():
        v = np.array(v)
        say(f"  {k:12s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  "
            f"p10-p90 {np.percentile(v, 10):8.3f} .. {np.percentile(v, 90):8.3f}   last loss {float(losses[k]):.4f}")
    ctc, again, fea = (float(np.median(res[k])) for k in ("ctc", "ctc (again)", "feature"))
    spread = abs(again - ctc)
    say(f"  spread between the two ctc legs {spread:.3f} ms ({100 * spread / ctc:.2f} %)")
    say(f"  feature - ctc = {fea - ctc:+.3f} ms/step   feature / ctc = {fea / ctc:.4f}")
    assert all(torch.isfinite(d).all() for d in deltas.values())
    del graphs                                          # before the buffers they point into


KERNEL_SHAPES = [(32, 499, 500, 768), (32, 499, 500, 1024)]      # (B, T, padded rows per clip, H)


def kernel_ab(say, calls=20, rounds=5):
    """paa_feature_cos alone: us per call and the bytes it moves over that time."""
    L, p = _lib.lib(), _lib.ptr
    say("paa_feature_cos alone (loss, d and the cotangent; HIP events, 20 calls, median of 5 rounds):")
    for B, T, P, H in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(5)
        h = torch.randn(B, P, H, generator=g).cuda()
        ref = torch.randn(B, T, H, generator=g).cuda()
        loss, dist, dh = torch.zeros(B, device="cuda"), torch.zeros(B, T, device="cuda"), torch.zeros(B, P, H, device="cuda")
        work = torch.zeros(int(L.paa_feature_cos_work_floats(B, T)), device="cuda")
        st = _lib.stream_ptr()
        res = []
        for rnd in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                _lib.check(L.paa_feature_cos(p(h), P, p(ref), T, None, B, T, H, 1.0, p(loss), p(dist), p(dh), p(work), st))
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res.append(e0.elapsed_time(e1) * 1e3 / calls)
        us = float(np.median(res))
        nbytes = 3 * B * T * H * 4
        say(f"  B {B:3d} T {T:4d} P {P:4d} H {H:5d}:  {us:8.1f} us per call (two launches)   {nbytes / 1e6:7.1f} MB moved   "
            f"{nbytes / us / 1e6:6.2f} TB/s   (finite: {bool(torch.isfinite(loss).all() and torch.isfinite(dh).all())})")
    say("  (operands of this size fit the 256 MiB last-level cache and the calls re-read them: the rate is no HBM rate, and a step, whose operands were just written, may see either)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--step_limit", type=float, default=20.0, help="seconds a single replay may take before the run stops")
    ap.add_argument("--no_kernels", action="store_true", help="skip the timing of paa_feature_cos alone")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    o = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for kind in ("universal", "clip"):
        step_ab(o, say, kind)
    if not o.no_kernels:
        kernel_ab(say)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
