"""No-GPU checks of the masking-threshold loss term: the float64 reference of tests/masking_loss_ref.py against
torch autograd and finite differences (it is the yardstick of the GPU tests), and the command-line surface."""
import os
import types

import numpy as np
import pytest
import torch

import masking_loss_ref as ML
import masking_ref as MR
from paa_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("L", [4096, 5000, 8737, 16000])
def test_reference_adjoint_is_the_gradient(L):
    B, amp = 2, 3e-2
    clean = synth.clean_audio(B, L, seed=7 if L in (4096, 5000) else 3)
    d = np.asarray(synth.normal(synth.key_of("mask0", 3), L), dtype=np.float64) * amp
    ths, pms = [], []
    for b in range(B):
        _, th, pm = MR.threshold(clean[b])
        ths.append(th)
        pms.append(pm)
    g, W, S = ML.grad(d, ths, pms)
    assert 0.1 < (W > 0).mean() < 0.95                             # the hinge is exercised on both sides
    dt = torch.tensor(d, requires_grad=True)
    loss = ML.torch_loss(dt, ths, pms)
    loss.backward()
    ga = dt.grad.numpy()
    assert abs(float(loss.detach()) - ML.loss_rows(S, ths, pms).sum()) <= 1e-12 * float(loss.detach())
    e = np.abs(g - ga).max() / np.abs(ga).max()
    print(f"L={L}: adjoint vs autograd {e:.2e}")
    assert e < 1e-6
    # central differences on 20 samples, the folded first and last 512 included
    rng = np.random.default_rng(L)
    idx = np.concatenate([[0, 1, 255, 256, 511, 512, 513], L - 1 - np.array([0, 1, 255, 256, 511, 512, 513]),
                          rng.integers(600, L - 600, 6)])
    assert idx.size == 20
    h = 1e-7
    f = lambda x: float(ML.torch_loss(torch.from_numpy(x), ths, pms))
    for i in idx:
        xp, xm = d.copy(), d.copy()
        xp[i] += h
        xm[i] -= h
        fd = (f(xp) - f(xm)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-4 * np.abs(g).max(), (L, i, fd, g[i])


def test_parser_and_naming():
    from paa_amd import attack_clips
    from paa_amd.training_utils import build, parser
    for make in (parser.create_arg_parser, attack_clips.create_arg_parser):
        a = make().parse_args([])
        assert a.masking_loss_alpha == 0.0 and isinstance(a.masking_loss_alpha, float)
        a = make().parse_args(["--norm_type", "linf", "--masking_loss_alpha", "2.5e-7"])
        assert a.masking_loss_alpha == 2.5e-7
    off = parser.create_arg_parser().parse_args(["--norm_type", "linf"])
    on = parser.create_arg_parser().parse_args(["--norm_type", "linf", "--masking_loss_alpha", "1e-6"])
    assert build.masking_loss_suffix(off) == "" and build.masking_loss_suffix(on) == "_ml1e-06"
    assert build.masking_loss_suffix(types.SimpleNamespace()) == ""                 # args without the attribute
    assert build.attack_size_string(on) == build.attack_size_string(off)             # results.json keeps a plain number
    float(build.attack_size_string(on))


def test_run_directory_names(tmp_path):
    from paa_amd.training_utils import build, parser
    names = {}
    for key, extra in (("off", []), ("on", ["--masking_loss_alpha", "1e-6"])):
        a = parser.create_arg_parser().parse_args(["--norm_type", "linf", "--silent", "--small_data",
                                                   "--logs_dir", str(tmp_path)] + extra)
        build.create_logger(a)
        names[key] = os.path.basename(a.save_dir)
    assert names["off"] == f"linf_{build.attack_size_string(a)}_untargeted_adam"     # the directory a run always had
    assert names["on"] == f"linf_{build.attack_size_string(a)}_ml1e-06_untargeted_adam"


def test_stepper_alpha_validation_needs_no_gpu():
    """set_masking_alpha's argument checks run before any device work."""
    from paa_amd.training_utils.pgd import PgdStepper
    st = PgdStepper.__new__(PgdStepper)
    st._alpha_captured, st.mask_alpha, st.alpha_dev = False, 0.0, None
    with pytest.raises(ValueError, match="after capture"):
        st.set_masking_alpha(1.0)
    with pytest.raises(ValueError, match=">= 0"):
        st.set_masking_alpha(-1.0)
    st.set_masking_alpha(0.0)
    assert st.mask_alpha == 0.0
