"""Cost of room responses on the placement layer (run on the GPU box).

1. paa_rir_draw and paa_rir_apply (forward and adjoint) alone at (32 x 160000) with K = 1024, 4096 and 16384 taps: us per call, HIP
   events over --reps calls, the calls alternating inside every round, median of --rounds; beside the two applies the achieved
   TFLOP/s of 2 B L (K + 31) flop against the 155 TF the f32-input MFMA reaches.
2. The 32 x 10 s fp32-parity step with --norm_type linf as replayed hipGraphs: the mode off next to the mode on (a synthetic bank
   of 64 responses, placement itself off) at the three K, alternating in one process; ms / step, spread and the on / off ratios.

On a library without the room-response entries (an older checkout) the tool times the off leg alone, so the same tool shows that
the off leg did not move.

    python tools/rir_step_ab.py [--steps 10] [--rounds 5] [--skip-kernel] [--skip-step]
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

TAPS = (1024, 4096, 16384)
N_ROOMS = 64
PEAK_TF = 155.0


def have_rir():
    return "paa_rir_apply" in _lib.exported_symbols()


def _args(dtype="fp32", taps=None):
    a = parser.create_arg_parser().parse_args(["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda",
                                               "--dtype", dtype, "--linf_size", "0.01"])
    if taps is not None:
        a.rir_bank, a.rir_count, a.rir_taps = "synthetic", N_ROOMS, taps
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
    from paa_amd.training_utils import rir
    lib = _lib.lib()
    B, L = o.batch, int(o.seconds * 16000)
    print(f"paa_rir_draw / paa_rir_apply at ({B} x {L}), {N_ROOMS} responses, {o.rounds} rounds of {o.reps} calls each, alternating, "
          f"HIP events (us per call; TF/s of 2 B L (K + 31) flop, of {PEAK_TF:g}):")
    x = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"G{b}", 3), L) for b in range(B)]).astype(np.float32)).cuda()
    y = torch.empty(B, L, device="cuda")
    index = torch.zeros(B, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for K in TAPS:
        bank = torch.from_numpy(rir.synthetic_bank(N_ROOMS, K, 16000, 0.2, 0.6, 6.0, 5)).cuda()
        st = _lib.stream_ptr()

        def apply(adjoint):
            return lambda: _lib.check(lib.paa_rir_apply(_lib.ptr(bank), N_ROOMS, K, _lib.ptr(index), _lib.ptr(x), _lib.ptr(y), B, L,
                                                        adjoint, st))
        calls = {"draw": lambda: _lib.check(lib.paa_rir_draw(5, _lib.ptr(counter), 0, 0, B, N_ROOMS, _lib.ptr(index), st)),
                 "apply": apply(0), "adjoint": apply(1)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(o.rounds):
            for k, fn in calls.items():
                ts[k].append(_events(fn, o.reps))
        flop = 2.0 * B * L * (K + 31)
        print(f"  K = {K}")
        for k, v in ts.items():
            med = float(np.median(v))
            rate = "" if k == "draw" else f"  {flop / med / 1e6:7.1f} TF/s ({100 * flop / med / 1e6 / PEAK_TF:.0f} %) of {flop / 1e9:.1f} GFLOP"
            print(f"    {k:7s} median {med:9.1f}  min {min(v):9.1f}  max {max(v):9.1f}{rate}")
        assert torch.isfinite(y).all()


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
    if have_rir():
        legs.update({f"on K={K}": K for K in TAPS})
    else:
        print("this library has no room-response entries: timing the off leg alone")
    # a captured graph holds raw pointers into its stepper's buffers and into the labels: every leg keeps its own alive for as long
    # as its graph is replayed
    graphs, deltas, steppers, labels = {}, {}, {}, {}
    for key, K in legs.items():
        args = _args(o.dtype, K)
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
          f"alternating (mode on: {N_ROOMS} synthetic responses, drawn per clip and step; placement off):")
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    o = ap.parse_args()
    if not o.skip_kernel and have_rir():
        kernel_timing(o)
    if not o.skip_step:
        step_ab(o)


if __name__ == "__main__":
    main()
