"""Cost of the alignment-margin loss on the universal step (run on the GPU box).

The 32 x 10 s base step, targeted, with --norm_type linf as replayed hipGraphs, alternating in one process:
  ctc, ctc (again)   --loss_type ctc, taken twice: the tool's own run-to-run spread
  margin             --loss_type margin (forced alignment + hinge in place of the CTC sequence)
ms / step (median over all timed steps), spread, and the margin / ctc ratio.  Every replay is synchronised and timed on its own,
and a step that takes longer than --step_limit seconds ends the run (nothing more is launched after it).

    python tools/margin_step_ab.py [--steps 10] [--rounds 5] [--dtype fp32] [--out profiles/margin_step_ab.txt]

After the step legs, the two loss sequences alone (paa_ctc_padded against paa_align_margin, both with dlogits and planes) on random
logits at 32 x 499 x 32 with 34, 150 and 248 label slots and at 16 x 1499 x 32 with 450: HIP events around 20 calls, median of 5
rounds, alternating.  --no_kernels skips this part.
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


def _args(dtype, loss_type, kappa):
    return parser.create_arg_parser().parse_args(
        ["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda", "--dtype", dtype, "--linf_size", "0.01",
         "--attack_mode", "targeted", "--loss_type", loss_type, "--margin_kappa", str(kappa)])


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
    a, B, L = A.BASE, o.batch, int(o.seconds * 16000)
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, o.dtype)
    legs = {"ctc": "ctc", "ctc (again)": "ctc", "margin": "margin"}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # every leg keeps its own stepper, perturbation and labels alive for as long as its graph is replayed (the graphs hold raw
    # pointers); a graph keeps the loss it was captured with, whatever the model's switch says at replay time
    graphs, deltas, steppers, labels, losses = {}, {}, {}, {}, {}
    for key, lt in legs.items():
        args = _args(o.dtype, lt, o.kappa)
        labels[key] = loss_helpers.make_labels(["ignored"] * B, None, args, B).to(device="cuda", dtype=torch.int32)
        deltas[key] = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
        steppers[key] = PgdStepper(m, args, L)
        graphs[key], r = steppers[key].capture(deltas[key], clean, labels[key])
        losses[key] = r["loss"]
    res = {k: [] for k in graphs}
    for rnd in range(o.rounds + 1):
        for k, g in graphs.items():
            ms = _timed(g.replay, o.steps, o.step_limit)
            if rnd:
                res[k] += ms
    say(f"universal step, {B} x {o.seconds:g} s, base, {o.dtype}, linf, targeted ({labels['ctc'].shape[1]} label slots, "
        f"{m.frames} frames), replayed graphs, {o.rounds} rounds of {o.steps} steps, alternating, every step synchronised:")
    for k, v in res.items():
        v = np.array(v)
        say(f"  {k:12s} median {np.median(v):8.3f} ms/step  min {v.min():8.3f}  max {v.max():8.3f}  "
            f"p10-p90 {np.percentile(v, 10):8.3f} .. {np.percentile(v, 90):8.3f}   last loss {float(losses[k]):.4f}")
    ctc, again, mar = (float(np.median(res[k])) for k in ("ctc", "ctc (again)", "margin"))
    spread = abs(again - ctc)
    say(f"  spread between the two ctc legs {spread:.3f} ms ({100 * spread / ctc:.2f} %)")
    say(f"  margin - ctc = {mar - ctc:+.3f} ms/step   margin / ctc = {mar / ctc:.4f}")
    say("  verdict: the margin leg is " + ("SLOWER than the ctc leg by more than that spread (first suspect: the backtrace)"
                                          if mar - max(ctc, again) > spread else "no slower than the ctc leg beyond that spread"))
    assert all(torch.isfinite(d).all() for d in deltas.values())
    del graphs                                          # before the buffers they point into
    if not o.no_kernels:
        loss_ab(say)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write("\n".join(lines) + "\n")


LOSS_SHAPES = [(32, 499, 32, 34), (32, 499, 32, 150), (32, 499, 32, 248), (16, 1499, 32, 450)]      # (B, T, V, S_max)


def loss_ab(say, calls=20, rounds=5):
    """The loss sequences alone: us per call of paa_ctc_padded and paa_align_margin on the same random logits and full label rows
    (every second id repeats its predecessor, as the lower-cased targets do)."""
    L, p = _lib.lib(), _lib.ptr
    say("loss sequences alone (dlogits + planes; HIP events, 20 calls, median of 5 rounds, alternating), us per call:")
    for B, T, V, S in LOSS_SHAPES:
        g = torch.Generator().manual_seed(5)
        z = (torch.randn(B, T, V, generator=g) * 2).cuda()
        lab = torch.randint(1, V, (B, S), generator=g, dtype=torch.int32)
        lab[:, 1::2] = lab[:, 0::2][:, : lab[:, 1::2].shape[1]]
        lab = lab.cuda()
        loss, dl = torch.zeros(B, device="cuda"), torch.zeros(B, T, V, device="cuda")
        hi, lo = (torch.zeros(B, T, V, dtype=torch.int16, device="cuda") for _ in range(2))
        wc = torch.zeros(int(L.paa_ctc_work_floats(B, T, V, S)), device="cuda")
        wm = torch.zeros(int(L.paa_align_margin_work_floats(B, T, V, S)), device="cuda")
        st = _lib.stream_ptr()
        run = {"ctc": lambda: _lib.check(L.paa_ctc_padded(p(z), p(lab), B, T, T, V, S, 0, -1.0, p(loss), p(dl), p(hi), p(lo), p(wc), st)),
               "margin": lambda: _lib.check(L.paa_align_margin(p(z), p(lab), None, B, T, T, V, S, 0, 1.0, -1.0, p(loss), None, p(dl),
                                                               p(hi), p(lo), p(wm), st))}
        res = {k: [] for k in run}
        for rnd in range(rounds + 1):
            for k, fn in run.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    res[k].append(e0.elapsed_time(e1) * 1e3 / calls)
        c, m = (float(np.median(res[k])) for k in ("ctc", "margin"))
        say(f"  B {B:3d} T {T:5d} V {V} S_max {S:4d}:  ctc {c:9.1f}  margin {m:9.1f}  margin / ctc = {m / c:.3f}   "
            f"(finite losses: {bool(torch.isfinite(loss).all())})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--step_limit", type=float, default=20.0, help="seconds a single replay may take before the run stops")
    ap.add_argument("--no_kernels", action="store_true", help="skip the timing of the loss sequences alone")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    step_ab(ap.parse_args())


if __name__ == "__main__":
    main()
