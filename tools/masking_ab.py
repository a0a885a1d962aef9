"""Cost of the masking norm (run on the GPU box).

1. paa_masking_threshold alone at (1, 160000), (32, 160000) and (16, 480000): us per call (HIP events over --reps calls, median
   of --rounds) and frames / s, plus the mean number of surviving maskers per frame (it sets the exp2 count of the threshold sum).
2. The per-clip step (ClipStepper) at 32 x 10 s, base, fp32-parity, replayed hipGraphs, alternating masking and max_phon in one
   process as tools/clip_step_ab.py does; prints ms / step and the masking / max_phon ratio.

    python tools/masking_ab.py [--steps 10] [--rounds 5] [--skip-threshold] [--skip-step]
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
from paa_amd.training_utils import build, parser
from paa_amd.training_utils.clip_attack import ClipStepper


def _args(norm, dtype="fp32"):
    return parser.create_arg_parser().parse_args(["--norm_type", norm, "--lr", "1e-4", "--optimizer_type", "pgd",
                                                  "--device", "cuda", "--dtype", dtype])


def _survivors(theta_call_args, x):
    """Mean maskers per frame: strict local maxima of P - Pmax + 96 that pass the quiet test and the 0.5-Bark suppression,
    recounted on the host from the device's levels (a sample of rows)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import masking_ref as MR
    from paa_amd.core.masking import masking_threshold
    _, _, pb = masking_threshold(x[:2], theta_call_args, psd=True)
    pb = pb.cpu().numpy()
    return float(np.mean([MR.threshold_from_pbar(pb[b], 16000)[2].mean() for b in range(pb.shape[0])]))


def threshold_timing(o):
    args = _args("masking")
    print(f"paa_masking_threshold (K1 level STFT + K2 threshold), {o.rounds} rounds of {o.reps} calls, HIP events:")
    for B, L in ((1, 160000), (32, 160000), (16, 480000)):
        x = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
        pr = runtime.get_proj(args, x.device, B, L)
        T, F = 1 + L // 256, 513
        theta = torch.empty(B, T, F, device="cuda")
        pmax = torch.empty(B, device="cuda")
        lib, st = _lib.lib(), _lib.stream_ptr()

        def call():
            _lib.check(lib.paa_masking_threshold(pr.h, _lib.ptr(x), B, L, None, _lib.ptr(theta), _lib.ptr(pmax), st))
        call()
        ts = []
        for _ in range(o.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(o.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / o.reps)
        us = float(np.median(ts))
        surv = _survivors(args, x)
        print(f"  ({B:2d}, {L:6d}): {B * T:6d} frames  median {us:9.1f} us  (min {min(ts):9.1f}, max {max(ts):9.1f})  "
              f"{B * T / us * 1e6:.3e} frames/s  maskers/frame {surv:.1f}")


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
    for norm in ("max_phon", "masking"):
        args = _args(norm, o.dtype)
        labels = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
        deltas[norm] = p.repeat(B, 1).contiguous()
        st = ClipStepper(m, args, L, None, build.init_phon_threshold_tensor(args))
        graphs[norm], _ = st.capture(deltas[norm], clean, labels)
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            ms = _time(g.replay, o.steps)
            if rnd:
                res[k].append(ms)
    print(f"per-clip step, {B} x {o.seconds:g} s, base, {o.dtype}, replayed graphs, {o.rounds} rounds of {o.steps} steps, alternating:")
    for k, v in res.items():
        v = np.array(v)
        print(f"  {k:9s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  spread {100 * (v.max() - v.min()) / np.median(v):.1f} %")
    print(f"  masking / max_phon = {np.median(res['masking']) / np.median(res['max_phon']):.4f}")
    assert all(torch.isfinite(d).all() for d in deltas.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--skip-threshold", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    o = ap.parse_args()
    if not o.skip_threshold:
        threshold_timing(o)
    if not o.skip_step:
        step_ab(o)


if __name__ == "__main__":
    main()
