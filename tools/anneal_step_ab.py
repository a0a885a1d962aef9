"""In-process A/B of the per-clip alpha schedule (run on the GPU box): replayed hipGraphs of one ClipStepper step at
32 x 10 s, base architecture, fp32-parity, linf 0.05, masking_loss_alpha 1e-5, device WER on, alternating rounds on one device —

    (a) off          the schedule off: paa_masking_loss with the scalar, today's sequence
    (b) off again    the same stepper built a second time: the spread of identical legs
    (c) on, nobody   the schedule on, targeted against a target no hypothesis equals: no clip ever succeeds, nothing is kept
    (d) on, all      the schedule on, untargeted against references no hypothesis equals: every clip succeeds at every step

then paa_clip_anneal alone at (32, 160000), HIP events, once with every row kept in every call and once with none.  Prints ms/step per
leg (median, min and max over the rounds) and the ratios (b)/(a), (c)/(a), (d)/(a).  ``--legs a`` runs on a tree without the schedule
(the parent commit's leg (a) for the same-box comparison).

    python tools/anneal_step_ab.py [--steps 10] [--rounds 5] [--legs a,b,c,d,entry]
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

OTHER = "zzz qqq jjj"
ALPHA0 = 1e-5
NAMES = {"a": "(a) off", "b": "(b) off again", "c": "(c) on, nobody", "d": "(d) on, all"}


def _time(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _line(k, v):
    v = np.array(v)
    return (f"  {k:16s} median {np.median(v):8.3f}  min {v.min():8.3f}  max {v.max():8.3f}  "
            f"spread {100 * (v.max() - v.min()) / np.median(v):.1f} %")


def _entry_alone(B, L, rounds, reps):
    """us per paa_clip_anneal call: every row kept in every call (losses fall from call to call) / no row kept (nobody succeeds)."""
    lib = _lib.lib()
    delta = torch.randn(B, L, device="cuda")
    best = torch.zeros(B, L, device="cuda")
    alpha, bloss, balpha = torch.full((B,), ALPHA0, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    bstep, step = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    losses = (torch.arange(reps, 0, -1, dtype=torch.float32, device="cuda")[:, None] * torch.ones(B, device="cuda")).contiguous()
    counts = {"every row kept": torch.tensor([[2, 2, 2]] * B, dtype=torch.int32, device="cuda"),
              "no row kept": torch.tensor([[0, 2, 2]] * B, dtype=torch.int32, device="cuda")}
    res = {k: [] for k in counts}
    for rnd in range(rounds + 1):
        for k, cnt in counts.items():
            bloss.fill_(float("inf"))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(reps):
                _lib.check(lib.paa_clip_anneal(_lib.ptr(delta), B, L, _lib.ptr(cnt), _lib.ptr(losses[i]), 0, 500, 20, 50, 1.2, 0.8,
                                               ALPHA0 / 100, ALPHA0 * 100, _lib.ptr(alpha), _lib.ptr(best), _lib.ptr(bloss),
                                               _lib.ptr(balpha), _lib.ptr(bstep), _lib.ptr(step), _lib.stream_ptr()))
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    print(f"paa_clip_anneal alone at ({B}, {L}), HIP events, {rounds} rounds of {reps} calls (us per call):")
    for k, v in res.items():
        print(_line(k, v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--legs", default="a,b,c,d,entry")
    o = ap.parse_args()
    legs = [k for k in o.legs.split(",") if k]
    a, B, L = A.BASE, o.batch, int(o.seconds * 16000)
    args = parser.create_arg_parser().parse_args(["--norm_type", "linf", "--linf_size", "0.05", "--lr", "1e-4", "--optimizer_type", "pgd",
                                                  "--device", "cuda", "--dtype", o.dtype, "--masking_loss_alpha", str(ALPHA0)])
    texts = [("the quick brown fox jumps over a lazy dog and runs " * 4)[:150] for _ in range(B)]
    labels = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, o.dtype)
    d0 = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(1e-2)).cuda().repeat(B, 1).contiguous()
    refs = loss_helpers.encode_refs([OTHER] * B)
    keep, variants = [], {}
    for k in legs:
        if k == "entry":
            continue
        kw = {}
        if k in "cd":
            from paa_amd.training_utils.clip_attack import AnnealConfig
            kw["anneal"] = AnnealConfig(1.2, 0.8, 20, 50, ALPHA0 / 100, ALPHA0 * 100, 500, k == "c")
        stp = ClipStepper(m, args, L, device_wer=True, **kw)
        stp.set_refs(refs)
        if kw:
            stp.anneal_reset(B)
        delta = d0.clone()
        g, _ = stp.capture(delta, clean, labels)
        keep.append((stp, delta))
        variants[NAMES[k]] = (g, stp)
    res = {k: [] for k in variants}
    for rnd in range(o.rounds + 1):
        for k, (g, stp) in variants.items():
            stp.stats_log.cursor.zero_()                       # nobody reads the per-step log here: keep it from filling
            ms = _time(g.replay, o.steps)
            if rnd:                                            # round 0 is the warm-up
                res[k].append(ms)
    print(f"{B} x {o.seconds:g} s, base, {o.dtype}, linf 0.05, masking_loss_alpha {ALPHA0:g}, device WER, replayed graphs, "
          f"{o.rounds} rounds of {o.steps} steps (ms/step):")
    for k, v in res.items():
        print(_line(k, v))
    med = {k: float(np.median(v)) for k, v in res.items()}
    for k in "bcd":
        if NAMES[k] in med and NAMES["a"] in med:
            print(f"  {NAMES[k]} / {NAMES['a']} = {med[NAMES[k]] / med[NAMES['a']]:.4f}")
    for k in "cd":
        if NAMES[k] in variants:
            stp = variants[NAMES[k]][1]
            print(f"  {NAMES[k]}: steps counted {int(stp.anneal_step.item())}, clips with a kept delta "
                  f"{int((stp.best_step[:B] >= 0).sum())} of {B}, alpha range [{float(stp.alpha_rows[:B].min()):.3e}, "
                  f"{float(stp.alpha_rows[:B].max()):.3e}]")
    for _, delta in keep:
        assert torch.isfinite(delta).all()
    if "entry" in legs:
        _entry_alone(B, L, o.rounds, 50)


if __name__ == "__main__":
    main()
