"""Cost of random placement of the universal perturbation (run on the GPU box).

1. paa_place_draw, paa_place_rows and paa_place_reduce alone at (32 x 160000) with Lp = 160000 and Lp = 16000: us per call, HIP
   events over --reps calls, the three calls alternating inside every round, median of --rounds; bytes moved / time beside the two
   memory-bound ones.
2. The 32 x 10 s fp32-parity step with --norm_type linf as replayed hipGraphs: placement off next to placement on (random shift,
   +-6 dB gain) with Lp = 160000 and Lp = 16000, alternating in one process; ms / step, spread and the on / off ratios.

On a library without the placement entries (an older checkout) the tool times the off leg alone, so the same tool shows that the
off leg did not move.

    python tools/place_step_ab.py [--steps 10] [--rounds 5] [--skip-kernel] [--skip-step]
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

LPS = (160000, 16000)


def have_placement():
    return "paa_place_rows" in _lib.exported_symbols()


def _args(dtype="fp32", seconds=None):
    a = parser.create_arg_parser().parse_args(["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda",
                                               "--dtype", dtype, "--linf_size", "0.01"])
    if seconds is not None:
        a.perturbation_seconds, a.place_shift, a.place_gain_db = seconds, "random", 6.0
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
    lib = _lib.lib()
    B, L = o.batch, int(o.seconds * 16000)
    print(f"paa_place_draw / paa_place_rows / paa_place_reduce at ({B} x {L}), {o.rounds} rounds of {o.reps} calls each, alternating, "
          "HIP events (us per call):")
    G = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"G{b}", 3), L) for b in range(B)]).astype(np.float32)).cuda()
    rows = torch.empty(B, L, device="cuda")
    shift = torch.zeros(B, dtype=torch.int32, device="cuda")
    gain = torch.ones(B, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for Lp in LPS:
        p = (torch.from_numpy(synth.perturbation(Lp, seed=5)) * np.float32(2e-3)).cuda()
        grad = torch.empty(Lp, device="cuda")
        st = _lib.stream_ptr()
        calls = {
            "draw": lambda: _lib.check(lib.paa_place_draw(5, _lib.ptr(counter), 0, 0, B, Lp, 1, 6.0, _lib.ptr(shift), _lib.ptr(gain), st)),
            "rows": lambda: _lib.check(lib.paa_place_rows(_lib.ptr(p), Lp, _lib.ptr(shift), _lib.ptr(gain), _lib.ptr(rows), B, L, st)),
            "reduce": lambda: _lib.check(lib.paa_place_reduce(_lib.ptr(G), _lib.ptr(shift), _lib.ptr(gain), _lib.ptr(grad), B, L, Lp, st)),
        }
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(o.rounds):
            for k, fn in calls.items():
                ts[k].append(_events(fn, o.reps))
        nbytes = {"draw": 0, "rows": 4 * (B * L + Lp), "reduce": 4 * (B * L + Lp)}
        print(f"  Lp = {Lp}")
        for k, v in ts.items():
            med = float(np.median(v))
            rate = f"  {nbytes[k] / med / 1e6:7.2f} TB/s of {nbytes[k] / 1e6:.1f} MB" if nbytes[k] else ""
            print(f"    {k:7s} median {med:9.1f}  min {min(v):9.1f}  max {max(v):9.1f}{rate}")


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
    legs = {"off": None}
    if have_placement():
        legs.update({f"on Lp={Lp}": Lp for Lp in LPS})
    else:
        print("this library has no placement entries: timing the off leg alone")
    # a captured graph holds raw pointers into its stepper's buffers and into the labels: every leg keeps its own alive for as long
    # as its graph is replayed (a freed block is handed to the next leg's allocations, and a label that is then read as some other
    # tensor's bits indexes the logits out of bounds)
    graphs, deltas, steppers, labels = {}, {}, {}, {}
    for key, Lp in legs.items():
        args = _args(o.dtype, None if Lp is None else Lp / 16000)
        labels[key] = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
        deltas[key] = (torch.from_numpy(synth.perturbation(Lp or L, seed=5)) * np.float32(2e-3)).cuda()
        steppers[key] = PgdStepper(m, args, L)
        graphs[key], _ = steppers[key].capture(deltas[key], clean, labels[key])
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            ms = _time(g.replay, o.steps)
            if rnd:
                res[k].append(ms)
    print(f"universal step, {B} x {o.seconds:g} s, base, {o.dtype}, linf, replayed graphs, {o.rounds} rounds of {o.steps} steps, "
          "alternating (placement on: random shift, +-6 dB gain):")
    for k, v in res.items():
        v = np.array(v)
        print(f"  {k:13s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  "
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    o = ap.parse_args()
    if not o.skip_kernel and have_placement():
        kernel_timing(o)
    if not o.skip_step:
        step_ab(o)


if __name__ == "__main__":
    main()
