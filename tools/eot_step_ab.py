"""Cost of the playback chain on the per-clip step (run on the GPU box).

The base model at 32 rows x 10 s, untargeted, --norm_type linf, as replayed hipGraphs, legs alternating in one process:
  plain, plain (again)   the per-clip step at B = 32 with the chain off, taken twice: the yardstick and the tool's own spread
  gain                   --eot_draws 4 at B = 8 (the same 32 model rows) with --place_gain_db 6
  gain+rooms             ... and --rir_bank synthetic at 4096 taps
  all                    ... and --drift_ppm 500 --noise_snr_db 20 30
ms / step (median over all timed steps), spread, and every leg's difference to the plain one.  Every replay is synchronised and
timed on its own, and a step that takes longer than --step_limit seconds ends the run (nothing more is launched after it).

    python tools/eot_step_ab.py [--steps 10] [--rounds 5] [--dtype fp32] [--out profiles/eot_step_ab.txt]

After the step legs, the three new launches alone at 8 x 4 x 160000 (paa_eot_rows with the per-row clean copy, paa_eot_reduce,
paa_eot_vote): HIP events around 50 calls, median of 5 rounds.  --no_kernels skips this part.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from paa_amd import _lib, arch as A, attack_clips, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils.clip_attack import ClipStepper

TEXTS = ["ab cd", "hello", "a b c", "xyz w"]
LEGS = {"plain": None, "plain (again)": None,
        "gain": ["--place_gain_db", "6"],
        "gain+rooms": ["--place_gain_db", "6", "--rir_bank", "synthetic", "--rir_taps", "4096"],
        "all": ["--place_gain_db", "6", "--rir_bank", "synthetic", "--rir_taps", "4096", "--drift_ppm", "500", "--noise_snr_db", "20", "30"]}


def _args(dtype, extra):
    return attack_clips.create_arg_parser().parse_args(
        ["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda", "--dtype", dtype, "--linf_size", "0.01",
         *extra])


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


def step_ab(o):
    a, R, G, L = A.BASE, o.rows, o.draws, int(o.seconds * 16000)
    m = PaaModel(a, A.rule_weights(a), R, L, o.dtype)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # every leg keeps its own stepper, perturbation, clips and labels alive for as long as its graph is replayed
    graphs, deltas, keep, losses = {}, {}, {}, {}
    for key, extra in LEGS.items():
        B = R if extra is None else R // G
        args = _args(o.dtype, [] if extra is None else ["--eot_draws", str(G), *extra])
        clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
        labels = loss_helpers.make_labels([TEXTS[b % 4] for b in range(B)], None, args, B)
        deltas[key] = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda().repeat(B, 1).contiguous()
        st = ClipStepper(m, args, L, eot_draws=0 if extra is None else G)
        graphs[key], r = st.capture(deltas[key], clean, labels)
        keep[key], losses[key] = (st, clean, labels), r["loss"]
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            ms = _timed(g.replay, o.steps, o.step_limit)
            if rnd:
                res[k] += ms
    say(f"per-clip step, {R} model rows x {o.seconds:g} s, base, {o.dtype}, linf, untargeted ({m.frames} frames): plain at B = {R}, the "
        f"chain at B = {R // G}, G = {G}; replayed graphs, {o.rounds} rounds of {o.steps} steps, alternating, every step synchronised:")
    for k, v in res.items():
        v = np.array(v)
        say(f"  {k:14s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  "
            f"p10-p90 {np.percentile(v, 10):8.3f} .. {np.percentile(v, 90):8.3f}   last loss {float(losses[k]):.4f}")
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = abs(med["plain (again)"] - med["plain"])
    say(f"  spread between the two plain legs {spread:.3f} ms ({100 * spread / med['plain']:.2f} %)")
    for k in ("gain", "gain+rooms", "all"):
        say(f"  {k:14s} - plain = {med[k] - med['plain']:+8.3f} ms/step   {k} / plain = {med[k] / med['plain']:.4f}")
    assert all(torch.isfinite(d).all() for d in deltas.values())
    del graphs                                          # before the buffers they point into
    if not o.no_kernels:
        kernels_ab(say, R // G, G, L)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def kernels_ab(say, B, G, L, calls=50, rounds=5):
    """The three new launches alone, us per call."""
    lib, p, R = _lib.lib(), _lib.ptr, B * G
    g = torch.Generator().manual_seed(5)
    clean, delta = torch.randn(B, L, generator=g).cuda(), (torch.randn(B, L, generator=g) * 1e-2).cuda()
    gain = torch.rand(R, generator=g).cuda() + 0.5
    rows, crow, grad = torch.empty(R, L, device="cuda"), torch.empty(R, L, device="cuda"), torch.empty(B, L, device="cuda")
    grows = torch.randn(R, L, generator=g).cuda()
    cnt = torch.randint(0, 9, (R, 3), generator=g, dtype=torch.int32).cuda()
    voted = torch.empty(B, 3, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()
    run = {"paa_eot_rows": lambda: _lib.check(lib.paa_eot_rows(p(clean), p(delta), p(gain), p(rows), p(crow), B, G, L, st)),
           "paa_eot_reduce": lambda: _lib.check(lib.paa_eot_reduce(p(grows), p(gain), p(grad), B, G, L, st)),
           "paa_eot_vote": lambda: _lib.check(lib.paa_eot_vote(p(cnt), B, G, 0, p(voted), st))}
    mb = {"paa_eot_rows": (2 * B + 2 * R) * L * 4 / 1e6, "paa_eot_reduce": (R + B) * L * 4 / 1e6, "paa_eot_vote": 0.0}
    say(f"the new launches alone at B = {B}, G = {G}, L = {L} (HIP events, {calls} calls, median of {rounds} rounds), us per call:")
    for k, fn in run.items():
        us = []
        for rnd in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                us.append(e0.elapsed_time(e1) * 1e3 / calls)
        t = float(np.median(us))
        say(f"  {k:15s} {t:9.1f} us" + (f"   ({mb[k]:.1f} MB moved, {mb[k] / t * 1e3:.0f} GB/s)" if mb[k] else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=32, help="model rows: the plain leg's batch, B * G of the others")
    ap.add_argument("--draws", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--step_limit", type=float, default=20.0, help="seconds a single replay may take before the run stops")
    ap.add_argument("--no_kernels", action="store_true", help="skip the timing of the new launches alone")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    step_ab(ap.parse_args())


if __name__ == "__main__":
    main()
