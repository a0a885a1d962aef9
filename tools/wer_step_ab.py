"""Cost of the on-device WER counters and what they buy the training loop (run on the GPU box).

(a) paa_argmax_ids + paa_wer_counts + paa_stats_push alone at (32, 499), (16, 1499) and a worst-case clip (T = 1499, letter and
    delimiter alternating: 750 hypothesis words against its own 750-word reference): us per call sequence, HIP events over
    --reps sequences, median of --rounds.
(b) train_epoch at 32 x 10 s, base, fp32-parity and bf16: --device_wer against the same loop without the flag (the host decode
    and edit distance after every step), whole epochs timed by wall clock, the two alternating in one process for --rounds
    rounds after one warm-up round; steps/s, spread, ratio.
(c) the bare replayed stepper (one captured hipGraph per step, what bench.py times) in the same process, next to (b).

    python tools/wer_step_ab.py [--steps 20] [--rounds 5] [--out profiles/wer_step_ab.txt]
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
from paa_amd.training_utils import parser, train
from paa_amd.training_utils.pgd import PgdStepper, StatsLog

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def _args(dtype, flag):
    return parser.create_arg_parser().parse_args(["--norm_type", "linf", "--lr", "1e-4", "--optimizer_type", "pgd", "--device", "cuda",
                                                  "--dtype", dtype, "--linf_size", "0.01"] + (["--device_wer"] if flag else []))


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def speechlike_ids(B, T, rng):
    out = np.zeros((B, T), dtype=np.int16)
    for b in range(B):
        row = []
        while len(row) < T:
            row += [int(rng.choice(list(range(5, 32)) + [4, 4, 4, 0, 0, 0, 0]))] * int(rng.integers(1, 5))
        out[b] = row[:T]
    return out


def kernel_timing(o):
    rng = np.random.default_rng(5)
    canon = loss_helpers.canon_table(None).cuda()
    lib, V = _lib.lib(), 32
    say(f"(a) paa_argmax_ids + paa_wer_counts + paa_stats_push, HIP events, {o.rounds} rounds of {o.reps} call sequences (us per sequence):")
    alt = np.full((1, 1499), 4, dtype=np.int16)
    alt[0, 0::2] = rng.choice([i for i in range(5, 32) if i != 27], size=750)
    cases = [("(32, 499) speech-like", speechlike_ids(32, 499, rng), None, loss_helpers.R_CAP),
             ("(16, 1499) speech-like", speechlike_ids(16, 1499, rng), None, loss_helpers.R_CAP),
             ("(1, 1499) worst case, 750 x 750 words", alt, None, 2048)]
    for name, ids, texts, r_cap in cases:
        B, T = ids.shape
        decoded = [t.lower() for t in loss_helpers.greedy_decode_ids(ids.tolist())]
        refs = loss_helpers.encode_refs(decoded if "worst" in name else [" ".join(t.split()[::-1]) for t in decoded], r_cap).cuda()
        logits = torch.full((B, T, V), -4.0)
        logits.scatter_(2, torch.from_numpy(ids.astype(np.int64))[..., None], 4.0)
        logits = logits.cuda()
        d_ids = torch.empty(B, T, dtype=torch.int16, device="cuda")
        rows = torch.empty(B, 3, dtype=torch.int32, device="cuda")
        stats = torch.zeros(8, device="cuda")
        log = StatsLog(torch.device("cuda"), 1 << 16)
        st = _lib.stream_ptr()
        calls = {
            "argmax": lambda: _lib.check(lib.paa_argmax_ids(_lib.ptr(logits), B * T, V, _lib.ptr(d_ids), st)),
            "wer_counts": lambda: _lib.check(lib.paa_wer_counts(_lib.ptr(d_ids), B, T, _lib.ptr(canon), V, _lib.ptr(refs), r_cap,
                                                                _lib.ptr(rows), _lib.ptr(stats[3:5]), st)),
            "stats_push": lambda: log.push(stats),
        }

        three = list(calls.values())

        def all3():
            for fn in three:
                fn()
        calls["all three"] = all3
        all3()
        torch.cuda.synchronize()
        log.read()
        ts = {k: [] for k in calls}
        for _ in range(o.rounds):
            for k, fn in calls.items():
                ts[k].append(_events(fn, o.reps))
            log.read()
        r = rows.cpu().numpy()
        say(f"  {name}: hypothesis words / clip max {r[:, 2].max()}, reference words max {r[:, 1].max()}, errors max {r[:, 0].max()}")
        for k, v in ts.items():
            say(f"    {k:10s} median {np.median(v):8.1f}  min {min(v):8.1f}  max {max(v):8.1f}")


def _loader(steps, B, L):
    texts = [("the quick brown fox jumps over a lazy dog and runs " * 4)[:150].strip() for _ in range(B)]
    xs = [torch.from_numpy(synth.clean_audio(B, L, seed=5, first_clip=i * B)).pin_memory() for i in range(min(steps, 4))]
    return [(xs[i % len(xs)], texts) for i in range(steps)], texts


def epoch_ab(o, dtype):
    a, B, L = A.BASE, o.batch, int(o.seconds * 16000)
    loader, texts = _loader(o.steps, B, L)
    m = PaaModel(a, A.rule_weights(a), B, L, dtype)
    p0 = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda().view(1, L)
    runs = {"host WER (no flag)": _args(dtype, False), "--device_wer": _args(dtype, True)}
    models = {k: PaaModel(a, A.rule_weights(a), B, L, dtype) for k in runs}       # train_epoch caches its stepper on the model
    # (c) the bare replayed stepper
    args = _args(dtype, False)
    labels = loss_helpers.make_labels(texts, None, args, B).to(device="cuda", dtype=torch.int32)
    pg = p0.clone()
    clean = loader[0][0].cuda()
    graph, _keep = PgdStepper(m, args, L).capture(pg, clean, labels)

    def bare():
        for _ in range(o.steps):
            graph.replay()
    fns = {k: (lambda k=k: train.train_epoch(runs[k], loader, p0.clone(), models[k], 0, None, None, None, None, None)) for k in runs}
    fns["bare replayed graph (bench.py's step)"] = bare
    res, last = {k: [] for k in fns}, {}
    for rnd in range(o.rounds + 1):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:
                res[k].append(o.steps / dt)
    say(f"(b, c) train_epoch, {B} x {o.seconds:g} s, base, {dtype}, pgd + linf, {o.steps} steps per epoch, wall clock around whole epochs, "
        f"{o.rounds} alternating rounds after one warm-up round (steps/s):")
    med = {}
    for k, v in res.items():
        v = np.array(v)
        med[k] = float(np.median(v))
        say(f"  {k:40s} median {np.median(v):7.2f}  min {v.min():7.2f}  max {v.max():7.2f}  spread {100 * (v.max() - v.min()) / np.median(v):.1f} %")
    h, d, b = med["host WER (no flag)"], med["--device_wer"], med["bare replayed graph (bench.py's step)"]
    say(f"  --device_wer / host WER = {d / h:.4f};  --device_wer / bare graph = {d / b:.4f};  host WER / bare graph = {h / b:.4f}")
    say(f"  per step: host WER {1e3 / h:.2f} ms, --device_wer {1e3 / d:.2f} ms, bare graph {1e3 / b:.2f} ms")
    r0, r1 = last["host WER (no flag)"], last["--device_wer"]
    say(f"  same scores on both routes: {(r0.avg_ctc, r0.avg_wer) == (r1.avg_ctc, r1.avg_wer)} (avg_ctc {r1.avg_ctc:.4f}, avg_wer {r1.avg_wer:.4f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wer_step_ab.txt"))
    o = ap.parse_args()
    say(f"tools/wer_step_ab.py on {torch.cuda.get_device_name(0)}")
    if not o.skip_kernel:
        kernel_timing(o)
    if not o.skip_epoch:
        for dtype in o.dtypes.split(","):
            epoch_ab(o, dtype)
    with open(o.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
