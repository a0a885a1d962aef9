"""CPU: the masking norm's reference (tests/masking_ref.py) against published values and its own invariants, and the host
plumbing of the norm (parser, params, run naming, error paths)."""
import argparse
import types

import numpy as np
import pytest

import masking_ref as MR
from paa_amd import _lib, runtime
from paa_amd.training_utils import build, parser, pgd, train

SR = 16000


def test_reference_values():
    assert float(MR.bark(1000.0)) == pytest.approx(8.5105, abs=1e-4)
    assert float(MR.quiet(1000.0)) == pytest.approx(-8.6309, abs=1e-4)
    z, q, ath, kA, lo, hi = MR.tables(SR)
    assert kA == 7 and z[6] <= 1.0 < z[7]
    assert np.isnan(ath[:kA]).all() and np.isfinite(ath[kA:]).all()
    width = hi - lo + 1
    assert width.min() >= 4 and width.max() <= 82 and width.min() == 4 and width.max() == 82
    assert np.all(lo <= np.arange(MR.F)) and np.all(hi >= np.arange(MR.F))


def _tone(k0, L=16384, amp=0.5):
    n = np.arange(L)
    return amp * np.sin(2 * np.pi * k0 * n / MR.N_FFT)


def test_pure_tone_single_masker_and_27_db_per_bark():
    k0 = 64                                                      # 1 kHz, centred on a bin
    x = _tone(k0)
    pbar, theta, pmax = MR.threshold(x, SR)
    _, _, nsurv, surv = MR.threshold_from_pbar(pbar, SR)
    inner = slice(4, pbar.shape[0] - 4)                         # frames clear of the reflect padding
    assert (nsurv[inner] == 1).all() and surv[inner][:, k0].all()
    z, q, ath, kA, _, _ = MR.tables(SR)
    t = pbar.shape[0] // 2
    below = np.arange(kA, k0 - 3)
    above_ath = theta[t, below] - ath[below] > 30.0
    b = below[above_ath]
    assert b.size >= 10
    slope = np.polyfit(z[b], theta[t, b], 1)[0]
    assert slope == pytest.approx(27.0, abs=0.05)


def test_survivors_half_bark_apart():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(8192) * 0.1 + _tone(40, 8192, 0.3) + _tone(45, 8192, 0.2) + _tone(150, 8192, 0.1)
    pbar, _, _ = MR.threshold(x, SR)
    _, _, nsurv, surv = MR.threshold_from_pbar(pbar, SR)
    z = MR.tables(SR)[0]
    assert nsurv.max() <= 43 and nsurv.max() > 5
    for t in range(surv.shape[0]):
        zs = z[np.nonzero(surv[t])[0]]
        assert np.all(np.diff(zs) >= 0.5)


def test_zero_clip_gives_ath():
    pbar, theta, pmax = MR.threshold(np.zeros(4096), SR)
    assert pmax == pytest.approx(-200.0)
    z, q, ath, kA, _, _ = MR.tables(SR)
    assert np.isneginf(theta[:, :kA]).all()
    np.testing.assert_allclose(theta[:, kA:], np.broadcast_to(ath[kA:], theta[:, kA:].shape), atol=1e-9)


def test_projection_reference_keeps_what_is_under_the_bound():
    rng = np.random.default_rng(5)
    d = rng.standard_normal(4096) * 1e-3
    T = 1 + 4096 // MR.HOP
    out = MR.project(d, np.full((T, MR.F), 1e9))
    valid = MR.HOP * (T - 1)
    np.testing.assert_allclose(out[:valid], d[:valid], atol=1e-8)
    assert (MR.project(d, np.zeros((T, MR.F))) == 0).all()


def test_parser_and_params():
    ap = parser.create_arg_parser()
    a = ap.parse_args(["--norm_type", "masking"])
    assert a.norm_type == "masking" and a.masking_margin_db == 0.0
    a = ap.parse_args(["--norm_type", "masking+l2", "--masking_margin_db", "-6"])
    assert a.norm_type == "masking+l2" and a.masking_margin_db == -6.0
    with pytest.raises(SystemExit):
        ap.parse_args(["--norm_type", "masking+nope"])
    a = ap.parse_args(["--norm_type", "masking", "--masking_margin_db", "-6"])
    prm = runtime.params_of(a)
    assert prm.norm_type == 7 == _lib.NORM_IDS["masking"] and prm.masking_margin_db == -6.0
    assert build.attack_size_string(a) == "-6.0"
    assert "masking_margin_db" in [f[0] for f in _lib.PaaParams._fields_][-1:]


def test_attack_clips_parser_inherits_masking():
    from paa_amd import attack_clips
    src = open(attack_clips.__file__).read()
    assert "create_arg_parser" in src
    a = parser.create_arg_parser().parse_args(["--norm_type", "masking", "--masking_margin_db", "3"])
    assert a.masking_margin_db == 3.0


def test_constraint_needs_clean():
    import torch
    args = types.SimpleNamespace(norm_type="masking", n_fft=1024, hop_length=256, win_length=1024, sr=16000,
                                 masking_margin_db=0.0)
    with pytest.raises(ValueError, match="clean_audio"):
        train.perturbation_constraint(torch.zeros(1, 4096), None, args, None, None)


def test_multi_rank_masking_refused():
    with pytest.raises(NotImplementedError, match="masking"):
        pgd.masking_route("masking", 2)
    with pytest.raises(NotImplementedError):
        pgd.masking_route("l2+masking", 4)
    pgd.masking_route("masking", 1)
    pgd.masking_route("snr", 2)
