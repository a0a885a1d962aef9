"""No GPU: the float64 attention reference of attn_ref.py agrees with torch autograd, and every score pattern the -m gpu
attention tests rely on does what its name claims."""
import numpy as np
import pytest
import torch

import attn_ref as R


def _head(name, T, seed=0):
    q, k, v = (x.astype(np.float64) for x in R.head_pattern(name, T, np.random.default_rng(seed)))
    return q, k, v


@pytest.mark.parametrize("T", [1, 2, 65, 499])
def test_reference_matches_autograd(T):
    rng = np.random.default_rng(T)
    q, k, v, do = (rng.standard_normal((T, R.HD)) * s for s in (1.5, 1.5, 1.0, 1.0))
    tq, tk, tv = (torch.from_numpy(x).requires_grad_(True) for x in (q, k, v))
    s = tq @ tk.T * R.SCALE
    o = torch.softmax(s, -1) @ tv
    o.backward(torch.from_numpy(do))
    ref = R.attn_ref(q, k, v, do)
    lse = (torch.logsumexp(s.detach(), -1) * R.LOG2E).numpy()
    for got, want in ((ref["o"], o.detach()), (ref["lse"], lse), (ref["dq"], tq.grad), (ref["dk"], tk.grad), (ref["dv"], tv.grad)):
        want = np.asarray(want)
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


@pytest.mark.parametrize("mode,lo,hi", [("bf16", 1e-4, 2e-2), ("split", 1e-7, 1e-4)])
def test_emulation_is_the_reference_up_to_its_rounding(mode, lo, hi):
    """On well-conditioned heads the emulating variant moves each output by about the mode's rounding, and no more."""
    T = 300
    inp = R.build_inputs(1, 2, T, T + 1, 320, mode == "split", seed=1, patterns=["random", "flat"])
    for h in range(2):
        q, k, v = R.head_slices(inp["qkv"][0], 2, h)
        a = R.attn_ref(q, k, v, inp["do"][0][:, h * R.HD:(h + 1) * R.HD])
        b = R.attn_emulated(*R.head_planes(inp, 0, 2, h), mode)
        assert abs(a["lse"] - b["lse"]).max() < (1e-9 if mode == "bf16" else 1e-4)     # split: lo*lo dropped in S
        for name in ("o", "dq", "dk", "dv"):
            if h == 1 and name == "dk":                        # Q = 0: dK is exactly 0 either way
                assert (a[name] == 0).all() and (b[name] == 0).all()
                continue
            e = np.abs(a[name] - b[name]).max() / np.abs(a[name]).max()
            assert e < hi and (h == 1 or e > lo), (h, name, e)  # flat: P is exactly 1 before normalising


def test_kappa_marks_saturated_heads():
    T = 499
    inp = R.build_inputs(1, 7, T, T + 1, 512, False, seed=2)
    kap = {}
    for h, pat in enumerate(inp["patterns"]):
        q, k, v = R.head_slices(inp["qkv"][0], 7, h)
        kap[pat] = R.attn_ref(q, k, v, inp["do"][0][:, h * R.HD:(h + 1) * R.HD])["kappa"]
    assert max(kap["random"].values()) < 10 and max(kap["flat"].values()) < 10
    assert min(kap["peaked"].values()) > 100 and kap["dominant_last"]["dk"] > 100 and kap["negshift"]["dq"] > 50


@pytest.mark.parametrize("T", [129, 499, 1499])
def test_rising_raises_the_lazy_max_late(T):
    q, k, _ = _head("rising", T)
    late, last = R.lazy_max_raises(R.scores2(q, k))
    nw = -(-T // R.WAVE)
    assert last == nw                                          # every wave raises inside the last (partial) tile
    assert late >= nw * len(R._jumps(T))                       # ... and at every earlier jump
    assert T % R.FWD_TILE != 0 and R._jumps(T)[-1] >= T // R.FWD_TILE * R.FWD_TILE


@pytest.mark.parametrize("T", [129, 499, 1499])
def test_falling_puts_the_maximum_first(T):
    q, k, _ = _head("falling", T)
    s2 = R.scores2(q, k)
    assert (s2.argmax(1) < R.FWD_TILE).all()
    assert R.lazy_max_raises(s2) == (0, 0)


@pytest.mark.parametrize("T", [2, 63, 499, 1499])
def test_peaked_rows_put_099_on_one_key(T):
    q, k, _ = _head("peaked", T)
    s2 = R.scores2(q, k)
    p = np.exp2(s2 - s2.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    assert p.max(1).min() > 0.99


@pytest.mark.parametrize("T", [1, 65, 1499])
def test_flat_rows_are_uniform(T):
    q, k, _ = _head("flat", T)
    s2 = R.scores2(q, k)
    p = np.exp2(s2 - s2.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    assert (p == 1.0 / T).all()


@pytest.mark.parametrize("T", [1, 65, 499, 1499])
def test_negshift_rows_have_lse_below_minus_128(T):
    q, k, v = _head("negshift", T)
    lse = R.attn_ref(q, k, v, np.zeros_like(v))["lse"]
    assert lse.max() < -128
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(np.exp2(-lse))).all()       # what a zero-filled key would give the dQ kernel


@pytest.mark.parametrize("T", [65, 499, 1499])
def test_dominant_last_key_wins_every_row(T):
    q, k, _ = _head("dominant_last", T)
    s2 = R.scores2(q, k)
    assert (s2.argmax(1) == T - 1).all()
    nw = -(-T // R.WAVE)
    assert R.lazy_max_raises(s2)[1] == nw                      # every wave raises its maximum in the masked tile


def test_build_inputs_layout():
    B, nh, T, P, Tp = 2, 3, 40, 45, 96
    for split in (False, True):
        inp = R.build_inputs(B, nh, T, P, Tp, split, seed=5)
        assert inp["patterns"] == [R.PATTERNS[i] for i in range(B * nh)]
        assert inp["qkv_hi"].shape == (B * P, 3 * nh * R.HD) and inp["do_hi"].shape == (B * P, nh * R.HD)
        planes = [inp[n] for n in ("qkv_hi", "qkv_lo", "do_hi", "do_lo") if inp[n] is not None]
        assert len(planes) == (4 if split else 2)
        for pl in planes:
            x = pl.reshape(B, P, -1)
            assert (x[:, T:] == R.NAN16).all() and not (x[:, :T] == R.NAN16).any()
        hi = R.bf16_to_f32(inp["qkv_hi"]).reshape(B, P, -1)[:, :T].astype(np.float64)
        lo = R.bf16_to_f32(inp["qkv_lo"]).reshape(B, P, -1)[:, :T] if split else 0.0
        assert np.array_equal(inp["qkv"], hi + lo)
        q, _, _ = R.head_slices(inp["qkv"][1], nh, 1)          # head (1, 1) is pattern 4: flat
        assert inp["patterns"][nh + 1] == "flat" and (q == 0).all()
