"""Cost of the masking-threshold loss term (run on the GPU box).

1. paa_masking_loss at (1 row, 32 x 160000), (32 rows, 32 x 160000) and (16 rows, 16 x 480000) next to paa_masking_threshold and
   the masking projection (paa_project_to / paa_project_rows, SOP_MASK) at the same shapes: us per call, HIP events over --reps
   calls, the three calls alternating inside every round, median of --rounds.  The loss and the projection calls both contain the
   threshold passes (K1 + K2); the difference to the threshold call is printed beside them.
2. The 32 x 10 s fp32-parity step with --norm_type linf, universal (PgdStepper) and per-clip (ClipStepper): alpha > 0 against the
   same step with alpha = 0, replayed hipGraphs alternating in one process; ms / step, spread and the ratio.

    python tools/masking_loss_ab.py [--steps 10] [--rounds 5] [--skip-kernel] [--skip-step]
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
from paa_amd.training_utils.pgd import PgdStepper


def _args(norm, dtype="fp32", alpha=0.0):
    return parser.create_arg_parser().parse_args(["--norm_type", norm, "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda",
                                                  "--dtype", dtype, "--linf_size", "0.01", "--masking_loss_alpha", str(alpha)])


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernel_timing(o):
    args = _args("masking")
    prm = runtime.params_of(args)
    lib = _lib.lib()
    print(f"paa_masking_loss next to paa_masking_threshold and the masking projection, {o.rounds} rounds of {o.reps} calls each, "
          "alternating, HIP events (us per call):")
    for rows, B, L in ((1, 32, 160000), (32, 32, 160000), (16, 16, 480000)):
        x = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
        d = (torch.from_numpy(np.stack([synth.normal(synth.key_of(f"mask{b}", 3), L) for b in range(rows)]).astype(np.float32))
             * np.float32(3e-2)).cuda()
        pr = runtime.get_proj(args, x.device, B, L)
        T, F = 1 + L // 256, 513
        theta, pmax = torch.empty(B, T, F, device="cuda"), torch.empty(B, device="cuda")
        grad, out = torch.zeros_like(d), torch.empty_like(d)
        lrow, lsum = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
        st = _lib.stream_ptr()
        calls = {
            "threshold": lambda: _lib.check(lib.paa_masking_threshold(pr.h, _lib.ptr(x), B, L, None, _lib.ptr(theta), _lib.ptr(pmax), st)),
            "loss": lambda: _lib.check(lib.paa_masking_loss(pr.h, prm, _lib.ptr(d), rows, _lib.ptr(x), B, L, None, _lib.ptr(grad),
                                                            _lib.ptr(lrow), _lib.ptr(lsum), None, st)),
            "projection": (lambda: _lib.check(lib.paa_project_to(pr.h, prm, _lib.ptr(d), _lib.ptr(out), 1, _lib.ptr(x), B, L, st)))
            if rows == 1 else
            (lambda: _lib.check(lib.paa_project_rows(pr.h, prm, _lib.ptr(d), _lib.ptr(out), rows, _lib.ptr(x), L, st))),
        }
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(o.rounds):
            for k, fn in calls.items():
                ts[k].append(_events(fn, o.reps))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        active = float((lrow > 0).float().mean())
        print(f"  ({rows:2d} rows, {B:2d} x {L:6d}), {B * T} clip frames, clips with loss > 0: {active:.2f}")
        for k, v in ts.items():
            extra = "" if k == "threshold" else f"  minus threshold {med[k] - med['threshold']:8.1f}"
            print(f"    {k:10s} median {med[k]:9.1f}  min {min(v):9.1f}  max {max(v):9.1f}{extra}")


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
    for name, cls in (("universal", PgdStepper), ("per-clip", ClipStepper)):
        graphs, deltas = {}, {}
        for key, alpha in (("alpha=0", 0.0), ("alpha>0", o.alpha)):
            args = _args("linf", o.dtype, alpha)
            labels = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
            deltas[key] = p.clone() if cls is PgdStepper else p.repeat(B, 1).contiguous()
            st = cls(m, args, L)
            graphs[key], _ = st.capture(deltas[key], clean, labels)
        res = {k: [] for k in graphs}
        for rnd in range(o.rounds + 1):
            for k, g in graphs.items():
                ms = _time(g.replay, o.steps)
                if rnd:
                    res[k].append(ms)
        print(f"{name} step, {B} x {o.seconds:g} s, base, {o.dtype}, linf, replayed graphs, {o.rounds} rounds of {o.steps} steps, "
              f"alternating (alpha {o.alpha:g}):")
        for k, v in res.items():
            v = np.array(v)
            print(f"  {k:8s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  "
                  f"spread {100 * (v.max() - v.min()) / np.median(v):.1f} %")
        print(f"  alpha>0 / alpha=0 = {np.median(res['alpha>0']) / np.median(res['alpha=0']):.4f}")
        assert all(torch.isfinite(d).all() for d in deltas.values())
        del graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--alpha", type=float, default=5e-6)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    o = ap.parse_args()
    if not o.skip_kernel:
        kernel_timing(o)
    if not o.skip_step:
        step_ab(o)


if __name__ == "__main__":
    main()
