"""In-process A/B of the attention backward: the dQ + dK/dV kernel pair (paa_attn_bwd_config(1)) against the one-pass kernel +
finish (paa_attn_bwd_config(2)), alternating in one process, HIP events around each attn_bwd call — run on the GPU box:

    python tools/attn_bwd_ab.py [B nh T]  >> profiles/attn_onepass_ab.txt

Default shape: the benchmark's (B = 32, nh = 12, T = 499, P = 500).  Both precisions; ROUNDS alternations of CALLS calls each
after a warm-up; per arm and round the mean, minimum and maximum per-call time.  Before timing, the two paths' outputs are
compared once (max |difference| over max |value| per tensor, and whether dK / dV agree bit for bit)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from paa_amd import _lib
from paa_amd.model import bf16_to_f32

ROUNDS, CALLS, WARM = 3, 50, 5
MODES = {1: "two kernels", 2: "one pass"}


def planes(x, split):
    """float32 tensor -> bf16 hi (and lo) planes as int16 device tensors (round-to-nearest-even through torch)."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16).view(torch.int16) if split else None
    return hi.view(torch.int16), lo


def main(B=32, nh=12, T=499):
    P, Tp, H = T + 1, -(-T // 32) * 32, nh * 64
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    g = torch.Generator(device="cuda").manual_seed(T)
    qkv = torch.randn(B * P, 3 * H, device="cuda", generator=g)
    do = torch.randn(B * P, H, device="cuda", generator=g)
    ws = torch.empty(L.paa_attn_dq_part_floats(B, nh, T, Tp), device="cuda")
    print(f"# B={B} nh={nh} T={T} P={P}: {ROUNDS} alternations x {CALLS} calls, us per attn_bwd call (mean / min / max)")
    for split in (True, False):
        qh, ql = planes(qkv, split)
        dh, dl = planes(do, split)
        ch, cl = torch.zeros(B * P, H, dtype=torch.int16, device="cuda"), (torch.zeros(B * P, H, dtype=torch.int16, device="cuda") if split else None)
        lse, delta = torch.zeros(B * nh, Tp, device="cuda"), torch.zeros(B * nh, Tp, device="cuda")
        if split:
            _lib.check(L.paa_attn_fwd_split(p(qh), p(ql), p(ch), p(cl), p(lse), B, T, P, Tp, H, nh, st))
        else:
            _lib.check(L.paa_attn_fwd(p(qh), p(ch), p(lse), B, T, P, Tp, H, nh, st))
        outs = {m: (torch.zeros(B * P, 3 * H, dtype=torch.int16, device="cuda"),
                    torch.zeros(B * P, 3 * H, dtype=torch.int16, device="cuda") if split else None) for m in MODES}

        def call(m):
            gh, gl = outs[m]
            _lib.check(L.paa_attn_bwd_ws(p(qh), p(ql), p(ch), p(cl), p(lse), p(dh), p(dl), p(delta), p(gh), p(gl), None, p(ws),
                                         B, T, P, Tp, H, nh, st))

        name = "split-bf16" if split else "bf16"
        for m in MODES:
            L.paa_attn_bwd_config(m)
            call(m)
        torch.cuda.synchronize()
        val = {m: sum(bf16_to_f32(x.cpu().numpy().view(np.uint16)).astype(np.float64) for x in outs[m] if x is not None) for m in MODES}
        for i, t in enumerate(("dQ", "dK", "dV")):
            a, r = (val[m].reshape(B, P, 3 * H)[:, :T, i * H:(i + 1) * H] for m in (2, 1))
            bits = all(x is None or torch.equal(x.view(B, P, 3 * H)[:, :T, i * H:(i + 1) * H], y.view(B, P, 3 * H)[:, :T, i * H:(i + 1) * H])
                       for x, y in zip(outs[2], outs[1]))
            print(f"{name}: {t} one pass against two kernels: max|diff| / max|value| {np.abs(a - r).max() / np.abs(r).max():.2e}, bit-equal {bits}")
        means = {m: [] for m in MODES}
        for rnd in range(-1, ROUNDS):            # round -1 warms the clocks and is not counted
            for m in MODES:
                L.paa_attn_bwd_config(m)
                for _ in range(WARM):
                    call(m)
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
                for a, b in ev:
                    a.record()
                    call(m)
                    b.record()
                torch.cuda.synchronize()
                us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
                if rnd < 0:
                    continue
                means[m].append(us.mean())
                print(f"{name} round {rnd} {MODES[m]:11s}: {us.mean():8.1f} / {us.min():8.1f} / {us.max():8.1f}", flush=True)
        L.paa_attn_bwd_config(0)
        m1, m2 = np.array(means[1]), np.array(means[2])
        spread = max(np.ptp(m1), np.ptp(m2))
        print(f"{name}: two kernels {m1.mean():.1f} us (spread {np.ptp(m1):.1f}), one pass {m2.mean():.1f} us (spread {np.ptp(m2):.1f}); "
              f"one pass - two kernels {m2.mean() - m1.mean():+.1f} us, 3 x largest spread {3 * spread:.1f} us")


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:4]))
