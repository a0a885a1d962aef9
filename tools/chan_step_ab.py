"""Cost of the playback channel on the placement layer (run on the GPU box).

1. paa_chan_draw, paa_drift_apply (forward and transpose) and paa_noise_add alone at (32 x 160000): us per call, HIP events over
   --reps calls, the calls alternating inside every round, median of --rounds; beside the passes the achieved GB/s of the
   2 B L floats each reads and writes (the noise: 3 B L, it reads the clean batch too).
2. The 32 x 10 s fp32-parity step with --norm_type linf as replayed hipGraphs, alternating in one process: the mode off (twice:
   the second off leg shows the spread between two graphs of the same step), drift alone, noise alone, both, and both with room
   responses of K = 4096 taps; ms / step, spread and the on / off ratios.

On a library without the channel entries (an older checkout) the tool times the off legs alone, so the same tool shows that the
off leg did not move.

    python tools/chan_step_ab.py [--steps 10] [--rounds 5] [--skip-kernel] [--skip-step]
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
from paa_amd.training_utils.pgd import PgdStepper

DRIFT_PPM, NOISE, TAPS, N_ROOMS = 20000.0, (20.0, 30.0), 4096, 64


def have_chan():
    return "paa_drift_apply" in _lib.exported_symbols()


def _args(dtype="fp32", drift=False, noise=False, rooms=False):
    a = parser.create_arg_parser().parse_args(["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda",
                                               "--dtype", dtype, "--linf_size", "0.01"])
    if drift:
        a.drift_ppm = DRIFT_PPM
    if noise:
        a.noise_snr_db = list(NOISE)
    if rooms:
        a.rir_bank, a.rir_count, a.rir_taps = "synthetic", N_ROOMS, TAPS
    return a


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernel_timing(o):
    from paa_amd.training_utils import channel
    B, L = o.batch, int(o.seconds * 16000)
    print(f"paa_chan_draw / paa_drift_apply / paa_noise_add at ({B} x {L}), {o.rounds} rounds of {o.reps} calls each, alternating, "
          f"HIP events (us per call; GB/s of the floats a pass reads and writes):")
    x = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"G{b}", 3), L) for b in range(B)]).astype(np.float32)).cuda()
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    ch = channel.Channel(x.device, B, L, 5, 0, DRIFT_PPM, NOISE)
    calls = {"draw": lambda: ch.draw(B), "drift": lambda: ch.apply(x, B), "transpose": lambda: ch.adjoint(x, B),
             "noise": lambda: ch.add_noise(ch.rows, clean, B)}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(o.rounds):
        for k, fn in calls.items():
            ts[k].append(_events(fn, o.reps))
    floats = {"draw": 0, "drift": 2, "transpose": 2, "noise": 3}
    for k, v in ts.items():
        med = float(np.median(v))
        rate = f"  {floats[k] * B * L * 4 / med / 1e3:7.1f} GB/s" if floats[k] else ""
        print(f"    {k:9s} median {med:9.1f}  min {min(v):9.1f}  max {max(v):9.1f}{rate}")
    assert torch.isfinite(ch.rows).all() and torch.isfinite(ch.grad_rows).all()


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
    legs = {"off": {}, "off again": {}}
    if have_chan():
        legs.update({"drift": dict(drift=True), "noise": dict(noise=True), "both": dict(drift=True, noise=True),
                     f"both + rooms K={TAPS}": dict(drift=True, noise=True, rooms=True)})
    else:
        print("this library has no channel entries: timing the off legs alone")
    # a captured graph holds raw pointers into its stepper's buffers and into the labels: every leg keeps its own alive for as long
    # as its graph is replayed
    graphs, deltas, steppers, labels = {}, {}, {}, {}
    for key, kw in legs.items():
        args = _args(o.dtype, **kw)
        labels[key] = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
        deltas[key] = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
        steppers[key] = PgdStepper(m, args, L)
        graphs[key], _ = steppers[key].capture(deltas[key], clean, labels[key])
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            ms = _time(g.replay, o.steps)
            if rnd:
                res[k].append(ms)
    print(f"universal step, {B} x {o.seconds:g} s, base, {o.dtype}, linf, replayed graphs, {o.rounds} rounds of {o.steps} steps, "
          f"alternating (drift {DRIFT_PPM:g} ppm, noise {NOISE[0]:g}-{NOISE[1]:g} dB, drawn per clip and step; placement off):")
    for k, v in res.items():
        v = np.array(v)
        print(f"  {k:22s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  "
              f"spread {100 * (v.max() - v.min()) / np.median(v):.1f} %")
    for k in res:
        if k != "off":
            print(f"  {k} / off = {np.median(res[k]) / np.median(res['off']):.4f}")
    assert all(torch.isfinite(d).all() for d in deltas.values())
    del graphs                                          # before the buffers they point into


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    o = ap.parse_args()
    if not o.skip_kernel and have_chan():
        kernel_timing(o)
    if not o.skip_step:
        step_ab(o)


if __name__ == "__main__":
    main()
