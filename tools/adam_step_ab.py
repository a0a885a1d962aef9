"""In-process A/B/C of the attack step at the headline shape (base architecture, 32 x 10 s, fp32, snr 40), interleaved rounds on
ONE device, timed with device events after warm-up:

    A  the PGD step replayed from its captured graph (PgdStepper.capture)
    B  the Adam step replayed from its captured graph (PgdStepper(optimizer=...): paa_adam_step instead of the sign step)
    C  the eager Adam sequence the Adam branch ran before: model.fwd_bwd + torch.optim.Adam.step + perturbation_constraint

Then B and C run N steps each from the same start (own optimizers, StepLR between steps) and their perturbations and moments are
compared.  Prints one JSON line.

    python tools/adam_step_ab.py [--steps 16] [--rounds 4] [--compare 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from paa_amd import arch as A, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils import build, parser
from paa_amd.training_utils.pgd import PgdStepper
from paa_amd.training_utils.train import perturbation_constraint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--compare", type=int, default=5)
    o = ap.parse_args()
    a, B, L = A.BASE, 32, 160000
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    texts = [("the quick brown fox jumps over a lazy dog and runs " * 4)[:150] for _ in range(B)]
    args = parser.create_arg_parser().parse_args(["--norm_type", "snr", "--snr_db", "40", "--lr", "1e-4", "--device", "cuda",
                                                  "--dtype", "fp32", "--optimizer_type", "adam", "--step_size", "1", "--gamma", "0.5"])
    labels = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    logits = torch.empty(B, m.frames, a.vocab_size, device="cuda")
    p0 = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda().view(1, L)

    def adam_pair():
        p = torch.nn.Parameter(p0.clone())
        opt, sched = build.create_optimizer(args, p)
        return p, opt, sched

    # A: PGD, graph
    pa = p0.clone()
    st_a = PgdStepper(m, args, L)
    ga, _ = st_a.capture(pa, clean, labels, logits_out=logits)
    # B: Adam on the device step, graph
    pb, opt_b, _ = adam_pair()
    st_b = PgdStepper(m, args, L, optimizer=opt_b)
    gb, _ = st_b.capture(pb.data, clean, labels, logits_out=logits)
    # C: the eager chain (train.py:165-175 as the Adam branch ran it)
    pc, opt_c, _ = adam_pair()

    def eager_adam(p, opt):
        r = m.fwd_bwd(clean, p.data, labels, st_a.direction)
        opt.zero_grad(set_to_none=True)
        p.grad = -r["grad"].view_as(p)
        opt.step()
        with torch.no_grad():
            p.data = perturbation_constraint(p.data, clean, args, None, None)

    runs = {"A_pgd_graph": ga.replay, "B_adam_graph": gb.replay, "C_adam_eager": lambda: eager_adam(pc, opt_c)}
    ms = {k: [] for k in runs}
    for rnd in range(o.rounds + 1):
        for k, fn in runs.items():
            for _ in range(2):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(o.steps):
                fn()
            e1.record()
            e1.synchronize()
            if rnd:                       # round 0 is warm-up
                ms[k].append(round(e0.elapsed_time(e1) / o.steps, 3))
    med = {k: float(np.median(v)) for k, v in ms.items()}

    # B vs C: the same N steps from the same start, StepLR between steps
    pb2, opt_b2, sched_b2 = adam_pair()
    st_b2 = PgdStepper(m, args, L, optimizer=opt_b2)
    gb2, _ = st_b2.capture(pb2.data, clean, labels, logits_out=logits)
    pc2, opt_c2, sched_c2 = adam_pair()
    for _ in range(o.compare):
        gb2.replay()
        sched_b2.step()
        eager_adam(pc2, opt_c2)
        sched_c2.step()
    torch.cuda.synchronize()
    sb, sc = opt_b2.state[pb2], opt_c2.state[pc2]
    scale = float(pc2.detach().abs().max())
    cmp = {"steps": o.compare, "p_bit_equal": bool(torch.equal(pb2.detach(), pc2.detach())),
           "exp_avg_bit_equal": bool(torch.equal(sb["exp_avg"], sc["exp_avg"])),
           "exp_avg_sq_bit_equal": bool(torch.equal(sb["exp_avg_sq"], sc["exp_avg_sq"])),
           "step_count": [float(sb["step"]), float(sc["step"])],
           "p_max_rel_diff": float((pb2.detach() - pc2.detach()).abs().max()) / scale}
    print(json.dumps({"shape": {"arch": "base", "batch": B, "samples": L, "dtype": "fp32", "norm": "snr 40"},
                      "steps_per_round": o.steps, "rounds": o.rounds, "ms_per_step": ms, "median_ms": med,
                      "B_minus_A_ms": round(med["B_adam_graph"] - med["A_pgd_graph"], 3),
                      "C_minus_B_ms": round(med["C_adam_eager"] - med["B_adam_graph"], 3), "B_vs_C": cmp}), flush=True)


if __name__ == "__main__":
    main()
