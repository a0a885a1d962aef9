"""CPU: the float64 statement of the feature-distance loss (tests/feature_ref.py) against torch's float64 autograd, its
degenerate-row rule, the flag, the two mode rules and the four C entries against the header."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import feature_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_feature_cos_work_floats", "paa_feature_cos", "paa_model_features", "paa_model_set_feature_loss")


def _rows(B, T, H, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal((B, T, H)), g.standard_normal((B, T, H)) * 3.0 + 0.25


@pytest.mark.parametrize("B,T,P,H,frames,gs", [(1, 1, 1, 4, None, 1.0), (3, 7, 9, 12, None, -1.0), (3, 7, 9, 12, [7, 3, 1], 2.5),
                                               (2, 24, 32, 64, [24, 19], 1.0)])
def test_reference_equals_float64_autograd(B, T, P, H, frames, gs):
    """loss and cotangent against autograd of (1 - cosine_similarity).sum() over the valid frames.  Both sides are float64 with a
    handful of operations per element and H-term dot products: rtol 1e-12 leaves three decades above H * 2^-53."""
    h, r = _rows(B, P, H, 5 + T)
    out = FR.feature_cos(h, r[:, :T], frames, gs, T)
    ht = torch.from_numpy(h).requires_grad_(True)
    d = 1.0 - F.cosine_similarity(ht[:, :T], torch.from_numpy(r[:, :T]), dim=-1, eps=0.0)
    fr = [T] * B if frames is None else frames
    keep = torch.arange(T)[None, :] < torch.tensor(fr)[:, None]
    loss = (d * keep).sum(dim=1)
    (gs * loss.sum()).backward()
    assert np.allclose(out["loss"], loss.detach().numpy(), rtol=1e-12, atol=0)
    assert np.allclose(out["dist"], (d * keep).detach().numpy(), rtol=1e-12, atol=1e-15)
    scale = np.abs(ht.grad.numpy()).max()
    assert np.allclose(out["dh"], ht.grad.numpy(), rtol=1e-12, atol=1e-12 * scale)
    # rows past T_b, and the pad rows of the padded layout, are exact zeros
    for b in range(B):
        assert not out["dh"][b, fr[b]:].any() and not out["dist"][b, fr[b]:].any()
        assert out["dh"][b, :fr[b]].any()
    assert list(out["frames"]) == fr


def test_degenerate_rows_have_distance_one_and_no_cotangent():
    h, r = _rows(2, 5, 8, 11)
    h[0, 1] = 0.0                     # |h| = 0
    r[1, 2] = 0.0                     # |r| = 0
    h[1, 4] = 1e-9 / np.sqrt(8.0)     # |h| = 1e-9 <= 1e-8
    r[0, 3] *= 2e-8 / np.linalg.norm(r[0, 3])      # |r| = 2e-8 > 1e-8: an ordinary row
    out = FR.feature_cos(h, r)
    for b, t in ((0, 1), (1, 2), (1, 4)):
        assert out["dist"][b, t] == 1.0 and not out["dh"][b, t].any(), (b, t)
    c = np.dot(h[0, 3], r[0, 3]) / (np.linalg.norm(h[0, 3]) * np.linalg.norm(r[0, 3]))
    assert abs(out["dist"][0, 3] - (1.0 - c)) < 1e-12 and out["dh"][0, 3].any()
    assert np.isfinite(out["dh"]).all() and np.isfinite(out["loss"]).all()
    # equal rows: distance 0 up to the rounding of the three dot products, cotangent of that order
    same = FR.feature_cos(h[:, :1], h[:, :1])
    assert np.abs(same["dist"]).max() <= 2.0 ** -50 and np.abs(same["dh"]).max() <= 2.0 ** -48
    # frame counts are clamped to [1, T]
    assert list(FR.feature_cos(h, r, [0, 99])["frames"]) == [1, 5]
    d32, l32 = FR.rounded(out)
    assert d32.dtype == np.float32 and l32.dtype == np.float32 and np.allclose(l32, out["loss"], rtol=2.0 ** -22)


# ---- flags and mode rules -----------------------------------------------------------------------------------------------------
def _args(**over):
    from paa_amd import attack_clips
    a = attack_clips.create_arg_parser().parse_args([])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_parser_accepts_feature_and_rejects_hinge():
    from paa_amd import attack_clips
    from paa_amd.training_utils import parser
    for make in (parser.create_arg_parser, attack_clips.create_arg_parser):
        assert make().parse_args([]).loss_type == "ctc"
        assert make().parse_args(["--loss_type", "feature"]).loss_type == "feature"
        assert make().parse_args(["--loss_type", "margin"]).loss_type == "margin"
        with pytest.raises(SystemExit):
            make().parse_args(["--loss_type", "hinge"])


def test_modes_feature_on_and_the_table():
    from paa_amd.training_utils import modes
    from paa_amd.training_utils.modes import FEATURE, RULES, Modes, check
    assert Modes.of().feature_on is False and Modes.of(_args(loss_type="margin")).feature_on is False
    m = Modes.of(_args(loss_type="feature"))
    assert m.feature_on is True and m.margin_on is False and m.loss_type == "feature"
    check(m, FEATURE + modes.MARGIN)
    # with the default flags neither rule is looked at
    check(Modes.of(_args(attack_mode="targeted", eot_draws=4)), FEATURE)
    assert FEATURE == ("feature_targeted", "feature_eot") and all(RULES[k].mode == "feature_on" for k in FEATURE)
    # no new dataclass field, and the EOT rules stay the last three of the table, the feature rules right before them
    assert list(Modes.__dataclass_fields__)[-1] == "search_on" and "feature_on" not in Modes.__dataclass_fields__
    assert list(RULES)[-3:] == list(modes.EOT) and list(RULES)[-5:-3] == list(FEATURE)


@pytest.mark.parametrize("flags,key,exc,msg", [
    (dict(attack_mode="targeted"), "feature_targeted", ValueError, "--loss_type feature does not run with --attack_mode targeted"),
    (dict(eot_draws=2, place_gain_db=6.0), "feature_eot", NotImplementedError, "--loss_type feature is not implemented with --eot_draws"),
])
def test_feature_refusals_by_rule_message_and_entry_point(flags, key, exc, msg):
    from paa_amd import attack_clips, run_attack
    from paa_amd.training_utils import modes
    a = _args(loss_type="feature", norm_type="snr", **flags)
    m = modes.Modes.of(a)
    assert modes.RULES[key].exc is exc and modes.RULES[key].when(m, modes.Ctx())
    with pytest.raises(exc, match=re.escape(msg)):
        modes.check(m, (key,))
    assert [k for k in modes.FEATURE if modes.RULES[k].when(m, modes.Ctx())][0] == key
    # the entry points raise it with their flag rules, before anything touches a GPU
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "is_available", lambda: False)
        with pytest.raises(exc, match=re.escape(msg)):
            attack_clips.main(a)
        if key == "feature_targeted":          # --eot_draws is a flag of attack_clips alone
            mp.setattr(torch.cuda, "is_available", lambda: True)
            with pytest.raises(exc, match=re.escape(msg)):
                run_attack.main(a)


def test_run_marks():
    from paa_amd.training_utils import build
    assert build.loss_suffix(_args()) == "" and build.loss_extra(_args()) == {}
    assert build.loss_suffix(_args(loss_type="margin")) == "" and build.loss_extra(_args(loss_type="margin")) == {}
    assert build.loss_suffix(_args(loss_type="feature")) == "_feature"
    assert build.loss_extra(_args(loss_type="feature")) == {"loss_type": "feature"}


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from paa_amd import _lib
    return _lib


def test_entries_declared_exported_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "paa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(paa_[a-z0-9_]+)\s*\(", hdr))
    L = lib.lib()
    for name in NEW_ENTRIES:
        assert name in declared and name in lib._SIGS and name in lib.exported_symbols() and hasattr(L, name), name
    assert L.paa_version() in lib.ABI_VERSIONS == (350, 351)
    assert [len(lib._SIGS[n][1]) for n in NEW_ENTRIES] == [2, 14, 8, 2]
    from paa_amd import build_ext
    assert "feat_kernels.hip" in build_ext.SOURCES
    # the work buffer: one float per frame, a multiple of four floats; an empty shape needs none
    assert L.paa_feature_cos_work_floats(32, 499) >= 32 * 499 and L.paa_feature_cos_work_floats(3, 7) % 4 == 0
    assert L.paa_feature_cos_work_floats(0, 7) == 0 and L.paa_feature_cos_work_floats(3, 0) == 0
    # a null model is refused by both model entries without touching a GPU
    assert L.paa_model_set_feature_loss(None, None) == lib.PAA_ERR_ARG
    assert L.paa_model_features(None, None, None, 1, 1, 1, None, None) == lib.PAA_ERR_ARG
