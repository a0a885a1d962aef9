"""No GPU: tests/conv0_ref.py's float64 statistics are torch's group_norm of conv1d in double, its signals and filter bank
stay the hard cases they are meant to be (a plain float32 evaluation stays accurate on them while some channel cancels by
1e4 and more), and forming the Gram products in float32 — what k_conv0_gram did before — loses three digits of rstd there."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv0_ref as R

LENGTHS = (8000, 10250)          # one Gram chunk; T0 = 2049 = a full chunk and a one-frame tail
EPS = 1e-5


@pytest.fixture(scope="module")
def bank():
    return R.filter_bank(32)


def test_filter_bank_and_signals_are_as_described(bank):
    assert bank.shape == (32, 10) and bank.dtype == np.float32
    assert np.array_equal(bank, R.filter_bank(32))
    assert np.abs(bank[8:16].sum(axis=1)).max() < 1e-6 and np.abs(bank[0:8].sum(axis=1)).min() > 1e-3
    assert np.all(bank[16:28].astype(np.float64).sum(axis=1) == 0)                   # differences cancel exactly
    assert [int((r != 0).sum()) for r in bank[16:24]] == [3] * 8 and [int((r != 0).sum()) for r in bank[24:28]] == [2] * 4
    assert np.all(bank[28:32] == bank[28:32, :1]) and np.all(bank[28:32] > 0)
    for L in LENGTHS:
        s = R.signals(L)
        assert list(s) == ["white", "tone120", "tone_dc", "chirp_gated", "lowpass", "dc_only", "zeros", "clipped"]
        assert all(v.dtype == np.float32 and v.shape == (L,) and np.abs(v).max() <= 1.0 for v in s.values())
        assert 0.4 < float((s["chirp_gated"] == 0).mean()) < 0.6
        assert np.all(s["zeros"] == 0) and np.all(s["dc_only"] == np.float32(0.3))
        assert float(np.abs(s["clipped"]).max()) == 1.0 and abs(float(np.abs(s["lowpass"]).max()) - 0.5) < 1e-6
    assert R.n_frames(8000) == 1599 and R.n_frames(10250) == R.C0_GCH + 1


@pytest.mark.parametrize("L", LENGTHS)
def test_stats64_is_torch_group_norm_in_double(bank, L):
    """num_groups == C, as HF's conv layer 0 uses it: group_norm(conv1d(x)) in double == (v - mean) * rstd of stats64."""
    W = torch.from_numpy(bank).double()[:, None, :]
    for name, x in R.signals(L).items():
        v = F.conv1d(torch.from_numpy(x).double()[None, None, :], W, stride=R.STRIDE)          # (1, C, T0)
        assert v.shape[-1] == R.n_frames(L)
        ref = F.group_norm(v, 32, eps=EPS)[0].numpy()
        mean, rstd = R.stats64(x, bank, EPS)
        got = (v[0].numpy() - mean[:, None]) * rstd[:, None]
        assert np.abs(got - ref).max() <= 1e-12, (name, np.abs(got - ref).max())
        # and the statistics themselves, against torch's own reductions
        assert np.abs(mean - v[0].mean(dim=1).numpy()).max() <= 1e-12 * max(1.0, float(np.abs(mean).max()))
        r_t = 1.0 / np.sqrt(v[0].var(dim=1, unbiased=False).numpy() + EPS)
        assert np.abs(rstd / r_t - 1.0).max() <= 1e-12, name


@pytest.mark.parametrize("L", LENGTHS)
def test_case_list_stays_hard_and_fair(bank, L):
    """Fair: a plain f32 evaluation keeps rstd to 5e-6 on every signal and every row of the bank (measured <= 9e-7), so the bound
    4 * e_32 + 5e-7 of the GPU test is a tight one.  Hard: on the tonal / DC clips some channel is 1e4 times smaller than the
    terms it is summed from."""
    for name, x in R.signals(L).items():
        _, e_r = R.stats_err(R.stats32(x, bank, EPS), R.stats64(x, bank, EPS), EPS)
        c = R.cancellation(x, bank)
        print(f"L={L} {name:12s} stats32 rstd err {e_r.max():.2e}  cancellation max {c.max():.1e}")
        assert e_r.max() <= 5e-6, (name, e_r.max())
        if name in R.TONAL:
            assert c.max() >= 1e4, (name, c.max())


@pytest.mark.parametrize("L", LENGTHS)
def test_f32_gram_products_lose_three_digits(bank, L):
    """Why tests/test_gpu_conv0_signals.py exists: with the products x_j * x_q rounded to f32 (and <= 8 of them summed in f32
    per thread) before the f64 reduction, w^T G w of a second-difference row on a 120 Hz tone is 1e6 times smaller than its
    terms and keeps their rounding: rstd is off by more than 1e-4 (measured 7e-4), where white noise gives 4e-9."""
    s = R.signals(L)
    out = {}
    for name in ("white", "tone120"):
        _, e = R.stats_err(R.gram_stats_f32_products(s[name], bank, EPS), R.stats64(s[name], bank, EPS), EPS)
        out[name] = e
        print(f"L={L} {name}: f32-product Gram rstd err, worst row {e.max():.2e}, second differences {e[R.SECOND_DIFF].max():.2e}")
    assert out["tone120"][R.SECOND_DIFF].max() > 1e-4
    assert out["white"].max() < 1e-7
