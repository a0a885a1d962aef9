"""Cost of true clip lengths on the universal step (run on the GPU box).

The 32 x 10 s base step with --norm_type linf as replayed hipGraphs, alternating in one process:
  off, off (again)   lengths off, taken twice: the tool's own run-to-run spread
  all = L            lengths on, every clip at the full length (the cost of the mode itself)
  mixed              lengths on, synthetic lengths uniform in [L/2, L] (build.synthetic_lengths): attention work scales with sum T_b^2
ms / step, spread, and the on / off ratios.  On a library without the length entries (an older checkout) the tool times the off legs
alone, so the same tool gives the yardstick on the parent commit.

    python tools/varlen_step_ab.py [--steps 10] [--rounds 5] [--dtype fp32] [--legs off,mixed]

--legs keeps only the named legs (off, off2, full, mixed), e.g. ONE leg under ``rocprofv3 --kernel-trace --stats`` for the attention
kernels' share of that leg (a run of its own: the profiler's overhead does not belong in the timings above).
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
from paa_amd.training_utils import build, parser
from paa_amd.training_utils.pgd import PgdStepper


def have_lengths():
    return "paa_model_set_lengths" in _lib.exported_symbols()


def _args(dtype):
    return parser.create_arg_parser().parse_args(["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda",
                                                  "--dtype", dtype, "--linf_size", "0.01"])


def _time(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def step_ab(o):
    a, B, L = A.BASE, o.batch, int(o.seconds * 16000)
    texts = [("the quick brown fox jumps over a lazy dog and runs " * 4)[:o.label_chars] for _ in range(B)]
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, o.dtype)
    legs = {"off": None, "off (again)": None}
    if have_lengths():
        mixed = build.synthetic_lengths(B, L, 5).tolist()
        legs.update({"all = L": [L] * B, "mixed": mixed})
        t = np.array([a.feat_lengths(n)[-1] for n in mixed], dtype=np.float64)
        print(f"mixed lengths: mean {np.mean(mixed) / L:.3f} L, sum T_b^2 / (B T_e^2) = {np.sum(t * t) / (B * a.feat_lengths(L)[-1] ** 2):.3f}")
    else:
        print("this library has no length entries: timing the off legs alone")
    if o.legs:
        names = {"off": "off", "off2": "off (again)", "full": "all = L", "mixed": "mixed"}
        legs = {names[k]: legs[names[k]] for k in o.legs.split(",") if names[k] in legs}
    # every leg keeps its own stepper, perturbation and labels alive for as long as its graph is replayed (the graphs hold raw
    # pointers); the length legs share the model's ONE length buffer, refilled before each leg's replays, outside the timed region
    graphs, deltas, steppers, labels = {}, {}, {}, {}
    for key, lengths in legs.items():
        args = _args(o.dtype)
        labels[key] = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
        deltas[key] = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
        steppers[key] = PgdStepper(m, args, L)
        graphs[key], _ = steppers[key].capture(deltas[key], clean, labels[key], **({} if lengths is None else {"lengths": lengths}))
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            if legs[k] is not None:
                m.set_lengths(legs[k])
            ms = _time(g.replay, o.steps)
            if rnd:
                res[k].append(ms)
    print(f"universal step, {B} x {o.seconds:g} s, base, {o.dtype}, linf, replayed graphs, {o.rounds} rounds of {o.steps} steps, alternating:")
    for k, v in res.items():
        v = np.array(v)
        print(f"  {k:13s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  "
              f"spread {100 * (v.max() - v.min()) / np.median(v):.1f} %")
    if "off" in res:
        off = np.median(res["off"])
        for k in res:
            if k != "off":
                print(f"  {k} / off = {np.median(res[k]) / off:.4f}")
    assert all(torch.isfinite(d).all() for d in deltas.values())
    del graphs                                          # before the buffers they point into


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--label_chars", type=int, default=60)      # feasible in the shortest mixed clip (T_b >= 249 frames)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--legs", default=None, help="comma list of off, off2, full, mixed (default: all)")
    step_ab(ap.parse_args())


if __name__ == "__main__":
    main()
