"""Cost of temporal masking of the masking threshold (run on the GPU box).

1. paa_masking_threshold at (1, 160000), (32, 160000) and (16, 480000) with the mode off and with --masking_post_ms 200
   --masking_pre_ms 20: us per call, HIP events over --reps calls, the legs alternating inside every round, median of --rounds.
   The mode-off leg runs twice per round ("off" and "off again"): the difference of two identical legs is the spread a ratio has
   to be read against.
2. The per-clip 32 x 10 s fp32-parity step with --norm_type masking (ClipStepper), mode off, on and off again: replayed hipGraphs
   alternating in one process; ms / step, spread and the ratio on / off.

    python tools/mask_time_ab.py [--steps 10] [--rounds 5] [--skip-kernel] [--skip-step]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils import parser
from paa_amd.training_utils.clip_attack import ClipStepper

LEGS = (("off", (0.0, 0.0)), ("on", (200.0, 20.0)), ("off again", (0.0, 0.0)))


def _args(times, dtype="fp32"):
    return parser.create_arg_parser().parse_args(["--norm_type", "masking", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda",
                                                  "--dtype", dtype, "--masking_post_ms", str(times[0]), "--masking_pre_ms", str(times[1])])


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _report(res, unit):
    med = {k: float(np.median(v)) for k, v in res.items()}
    for k, v in res.items():
        v = np.array(v)
        print(f"    {k:10s} median {med[k]:10.3f} {unit}  min {v.min():10.3f}  max {v.max():10.3f}  "
              f"spread {100 * (v.max() - v.min()) / med[k]:.1f} %")
    print(f"    on / off = {med['on'] / med['off']:.4f}   off again / off = {med['off again'] / med['off']:.4f}   "
          f"on - off = {med['on'] - med['off']:.3f} {unit}")


def kernel_timing(o):
    lib = _lib.lib()
    print(f"paa_masking_threshold, mode off / 200-20 / off again, {o.rounds} rounds of {o.reps} calls each, alternating, HIP events (us per call):")
    for B, L in ((1, 160000), (32, 160000), (16, 480000)):
        x = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
        T, F = 1 + L // 256, 513
        theta, pmax = torch.empty(B, T, F, device="cuda"), torch.empty(B, device="cuda")
        st = _lib.stream_ptr()
        calls, outs = {}, {}
        for key, times in LEGS:
            pr = runtime.get_proj(_args(times), x.device, B, L)
            calls[key] = (lambda h=pr.h: _lib.check(lib.paa_masking_threshold(h, _lib.ptr(x), B, L, None, _lib.ptr(theta), _lib.ptr(pmax), st)))
            calls[key]()
            torch.cuda.synchronize()
            outs[key] = theta.clone()
        assert torch.equal(outs["off"], outs["off again"]) and bool((outs["on"] >= outs["off"]).all())
        rose = float((outs["on"] > outs["off"]).float().mean())
        ts = {k: [] for k in calls}
        for _ in range(o.rounds):
            for k, fn in calls.items():
                ts[k].append(_events(fn, o.reps))
        print(f"  ({B:2d} x {L:6d}), {B * T} frames, {4 * B * T * F / 1e6:.1f} MB per plane, cells that rise: {100 * rose:.1f} %")
        _report(ts, "us")


def _time(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def step_ab(o):
    a, B, L = A.BASE, o.batch, int(o.seconds * 16000)
    texts = [("the quick brown fox jumps over a lazy dog and runs " * 4)[:150] for _ in range(B)]
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, o.dtype)
    p = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
    graphs, deltas = {}, {}
    for key, times in LEGS:
        args = _args(times, o.dtype)
        labels = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
        deltas[key] = p.repeat(B, 1).contiguous()
        graphs[key], _ = ClipStepper(m, args, L).capture(deltas[key], clean, labels)
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            ms = _time(g.replay, o.steps)
            if rnd:
                res[k].append(ms)
    print(f"per-clip step, {B} x {o.seconds:g} s, base, {o.dtype}, masking norm, replayed graphs, {o.rounds} rounds of {o.steps} steps, alternating:")
    _report(res, "ms")
    assert all(torch.isfinite(d).all() for d in deltas.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    o = ap.parse_args()
    if not o.skip_kernel:
        kernel_timing(o)
    if not o.skip_step:
        step_ab(o)


if __name__ == "__main__":
    main()
