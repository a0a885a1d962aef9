"""No-GPU checks of the per-clip adaptive masking-loss weight: the numpy statement of the decide / keep / move rule
against hand-written cases, AnnealConfig and the new refusals by rule key and message, the flags and the derived clamps, the records
and the summary with and without the new fields, and the two new C-ABI entries (declared, exported, bound, refusing bad arguments
before any launch)."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

import anneal_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_masking_loss_rows", "paa_clip_anneal")
F = np.float32
OK, FAIL = (2, 2, 2), (0, 2, 2)          # untargeted at wer_milli 500: WER 1 and WER 0


def _state(B, L=4, alpha=1e-5):
    return dict(alpha=np.full(B, alpha, dtype=F), best=np.full((B, L), -7.0, dtype=F), best_loss=np.full(B, np.inf, dtype=F),
                best_alpha=np.full(B, 9.0, dtype=F), best_step=np.full(B, -1, dtype=np.int32))


def _call(delta, counts, loss, st, step, targeted=False, up_every=2, down_every=3, up=1.2, down=0.8, lo=1e-7, hi=1e-3):
    out = AR.clip_anneal(delta, counts, loss, targeted, 500, up_every, down_every, up, down, lo, hi, st["alpha"], st["best"],
                         st["best_loss"], st["best_alpha"], st["best_step"], step)
    return dict(zip(("alpha", "best", "best_loss", "best_alpha", "best_step"), out[:5])), out[5]


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def test_keep_is_strict_and_nan_never_keeps():
    B, L = 5, 4
    delta = np.arange(B * L, dtype=F).reshape(B, L)
    st = _state(B, L)
    st["best_loss"][:] = [np.inf, 2.0, 2.0, 2.0, 2.0]
    st["best_step"][:] = [-1, 0, 0, 0, 0]
    loss = np.array([5.0, 1.5, 2.0, 2.5, np.nan], dtype=F)     # first success, lower, equal, higher, NaN
    new, step = _call(delta, [OK] * B, loss, st, 4)
    assert step == 5
    assert new["best_step"].tolist() == [4, 4, 0, 0, 0]
    assert new["best_loss"].tolist() == [5.0, 1.5, 2.0, 2.0, 2.0]
    assert np.array_equal(new["best"][:2], delta[:2]) and np.all(new["best"][2:] == -7.0)      # a tie keeps the earlier delta
    assert new["best_alpha"].tolist() == [F(1e-5), F(1e-5), 9.0, 9.0, 9.0]
    # a failing clip keeps nothing, whatever its loss
    new, _ = _call(delta, [FAIL] * B, np.zeros(B, dtype=F), st, 4)
    assert new["best_step"].tolist() == [-1, 0, 0, 0, 0] and np.all(new["best"] == -7.0)
    # a NaN loss against +inf does not keep either
    new, _ = _call(delta[:1], [OK], np.array([np.nan], dtype=F), _state(1, L), 0)
    assert new["best_step"].tolist() == [-1] and np.isinf(new["best_loss"][0])


def test_best_alpha_is_the_alpha_before_it_moves():
    delta = np.ones((1, 4), dtype=F)
    new, _ = _call(delta, [OK], np.array([1.0], dtype=F), _state(1), 1)          # n = 2: a raise and a keep in one call
    assert new["best_alpha"][0] == F(1e-5) and new["alpha"][0] == F(F(1e-5) * F(1.2))


def test_period_arithmetic():
    delta = np.zeros((2, 4), dtype=F)
    loss = np.array([1.0, 1.0], dtype=F)
    a0, up, dn = F(1e-5), F(F(1e-5) * F(1.2)), F(F(1e-5) * F(0.8))
    counts = [OK, FAIL]
    # n = 1 is on no period but 1
    assert _call(delta, counts, loss, _state(2), 0)[0]["alpha"].tolist() == [a0, a0]
    assert _call(delta, counts, loss, _state(2), 0, up_every=1)[0]["alpha"].tolist() == [up, a0]
    assert _call(delta, counts, loss, _state(2), 0, down_every=1)[0]["alpha"].tolist() == [a0, dn]
    # up_every = 1 raises at every step
    st, step = _state(2), 0
    for _ in range(3):
        st, step = _call(delta, counts, loss, st, step, up_every=1, down_every=100)
    assert st["alpha"][0] == F(F(up * F(1.2)) * F(1.2)) and st["alpha"][1] == a0 and step == 3
    # n = 2: the success period only; n = 3: the failure period only; n = 6: both coincide, each clip moves ITS way once
    assert _call(delta, counts, loss, _state(2), 1)[0]["alpha"].tolist() == [up, a0]
    assert _call(delta, counts, loss, _state(2), 2)[0]["alpha"].tolist() == [a0, dn]
    assert _call(delta, counts, loss, _state(2), 5)[0]["alpha"].tolist() == [up, dn]
    assert _call(delta, counts, loss, _state(2), 4)[0]["alpha"].tolist() == [a0, a0]


def test_products_are_float32_and_clamped_at_both_ends():
    a = AR.move_alpha([1e-5], 1.2, 1e-7, 1e-3)
    assert a.dtype == np.float32 and a[0] == F(1e-5) * F(1.2) and a[0] != F(np.float64(F(1e-5)) * 1.2 * (1 + 1e-9))
    a2 = AR.move_alpha(a, 1.2, 1e-7, 1e-3)
    assert a2[0] == F(a[0] * F(1.2))                                     # rounded after every product
    assert AR.move_alpha([9e-4], 1.2, 1e-7, 1e-3)[0] == F(1e-3)          # 1.08e-3 > alpha_max
    assert AR.move_alpha([1e-3], 1.2, 1e-7, 1e-3)[0] == F(1e-3)          # stays on it
    assert AR.move_alpha([1.1e-7], 0.8, 1e-7, 1e-3)[0] == F(1e-7)        # 0.88e-7 < alpha_min
    assert AR.move_alpha([1e-7], 0.8, 1e-7, 1e-3)[0] == F(1e-7)
    s = np.array([1e-5], dtype=F)
    for _ in range(40):
        s = AR.move_alpha(s, 0.8, 1e-7, 1e-3)
    assert s[0] == F(1e-7)
    for _ in range(80):
        s = AR.move_alpha(s, 1.2, 1e-7, 1e-3)
    assert s[0] == F(1e-3)
    assert AR.move_alpha([1e-5], 1.2, 1e-5, 1e-5)[0] == F(1e-5)          # alpha_min == alpha_max: alpha never moves


def test_targeted_success_and_inputs_left_alone():
    B, L = 3, 4
    delta = np.arange(B * L, dtype=F).reshape(B, L)
    st = _state(B, L)
    before = {k: v.copy() for k, v in st.items()}
    loss = np.array([1.0, 1.0, 1.0], dtype=F)
    counts = [(0, 2, 2), (1, 2, 2), (0, 0, 0)]                  # the transcript exactly; one error; an empty reference
    new, step = _call(delta, counts, loss, st, 5, targeted=True)
    assert new["best_step"].tolist() == [5, -1, -1] and step == 6
    assert new["alpha"].tolist() == [F(F(1e-5) * F(1.2)), F(F(1e-5) * F(0.8)), F(F(1e-5) * F(0.8))]
    for k, v in st.items():
        assert np.array_equal(v, before[k]), k
    assert np.array_equal(delta, np.arange(B * L, dtype=F).reshape(B, L)) and loss.tolist() == [1.0, 1.0, 1.0]


# ---- modes, refusals, flags -----------------------------------------------------------------------------------------------------
def _args(**kw):
    from paa_amd import attack_clips
    a = attack_clips.create_arg_parser().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


QIN = dict(alpha_search="qin", masking_loss_alpha=1e-5, norm_type="linf")


def test_flags_and_defaults():
    from paa_amd import attack_clips
    from paa_amd.training_utils import parser
    a = attack_clips.create_arg_parser().parse_args([])
    assert (a.alpha_search, a.alpha_up, a.alpha_down, a.alpha_up_every, a.alpha_down_every) == ("off", 1.2, 0.8, 20, 50)
    assert (a.alpha_min, a.alpha_max, a.stage1_steps) == (None, None, None)
    a = attack_clips.create_arg_parser().parse_args(["--alpha_search", "qin", "--alpha_up", "1.5", "--alpha_down", "0.5",
                                                     "--alpha_up_every", "2", "--alpha_down_every", "3", "--alpha_min", "1e-6",
                                                     "--alpha_max", "1e-2", "--stage1_steps", "7"])
    assert (a.alpha_search, a.alpha_up, a.alpha_down, a.alpha_up_every, a.alpha_down_every, a.alpha_min, a.alpha_max,
            a.stage1_steps) == ("qin", 1.5, 0.5, 2, 3, 1e-6, 1e-2, 7)
    with pytest.raises(SystemExit):
        attack_clips.create_arg_parser().parse_args(["--alpha_search", "linear"])
    u = parser.create_arg_parser().parse_args([])               # the universal runner does not get the flags
    assert not any(hasattr(u, k) for k in ("alpha_search", "alpha_up", "alpha_min", "stage1_steps"))


def test_modes_record():
    from paa_amd.training_utils.modes import Modes
    assert Modes.of(_args()).anneal_on is False and Modes.of(_args(**QIN)).anneal_on is True
    assert Modes.__dataclass_fields__["anneal_on"].default is False
    ns = types.SimpleNamespace(norm_type="snr")
    assert Modes.of(ns).anneal_on is False and Modes.of(ns, alpha_search="qin").anneal_on is True


def test_anneal_config_of_flags_and_bad():
    from paa_amd.training_utils.modes import AnnealConfig
    assert AnnealConfig.of(_args()) is None
    c = AnnealConfig.of(_args(**QIN))
    assert c == AnnealConfig(1.2, 0.8, 20, 50, 1e-5 / 100.0, 1e-5 * 100.0, 500, False) and c.bad() is None and c.bad(1e-5) is None
    c = AnnealConfig.of(_args(**QIN, alpha_min=2e-6, alpha_max=5e-5, search_success_wer=0.3336, attack_mode="targeted"))
    assert (c.alpha_min, c.alpha_max, c.wer_milli, c.targeted) == (2e-6, 5e-5, 334, True)
    ok = AnnealConfig(1.2, 0.8, 20, 50, 1e-7, 1e-3, 500, False)
    for kw, msg in ((dict(up=1.0), "alpha_up"), (dict(up=float("inf")), "alpha_up"), (dict(up=float("nan")), "alpha_up"),
                    (dict(down=1.0), "alpha_down"), (dict(down=0.0), "alpha_down"), (dict(up_every=0), "alpha_up_every"),
                    (dict(down_every=0), "alpha_down_every"), (dict(up_every=2.5), "alpha_up_every"),
                    (dict(alpha_min=0.0), "alpha_min"), (dict(alpha_min=1e-2), "alpha_min"), (dict(alpha_max=float("inf")), "alpha_max"),
                    (dict(alpha_min=float("nan")), "alpha_min"), (dict(wer_milli=0), "search_success_wer")):
        assert msg in ok._replace(**kw).bad(), kw
    assert "enclose" in ok.bad(1e-2) and "enclose" in ok.bad(1e-8) and ok.bad(1e-7) is None and ok.bad(1e-3) is None


@pytest.mark.parametrize("flags,key,exc,msg", [
    (dict(masking_loss_alpha=0.0), "anneal_alpha0", ValueError, "needs --masking_loss_alpha > 0"),
    (dict(alpha_up=1.0), "anneal_range", ValueError, "alpha_up must be finite and > 1, got 1.0"),
    (dict(alpha_down=1.0), "anneal_range", ValueError, r"alpha_down must lie in \(0, 1\), got 1.0"),
    (dict(alpha_up_every=0), "anneal_range", ValueError, "alpha_up_every must be an integer >= 1, got 0"),
    (dict(alpha_down_every=-3), "anneal_range", ValueError, "alpha_down_every must be an integer >= 1, got -3"),
    (dict(alpha_min=0.0), "anneal_range", ValueError, "need 0 < alpha_min <= alpha_max < inf"),
    (dict(alpha_min=1e-4), "anneal_range", ValueError, "the clamps must enclose the starting weight"),
    (dict(alpha_max=1e-6), "anneal_range", ValueError, "the clamps must enclose the starting weight"),
    (dict(stage1_steps=3), "anneal_stage", ValueError, "--stage1_steps applies to the two-stage run"),
    (dict(bound_search="shrink", stage1_steps=0, pgd_steps=8), "anneal_stage", ValueError, r"must lie in \[1, pgd_steps - 1\]"),
    (dict(bound_search="shrink", stage1_steps=8, pgd_steps=8), "anneal_stage", ValueError, r"must lie in \[1, pgd_steps - 1\]"),
    (dict(bound_search="shrink", pgd_steps=1), "anneal_stage", ValueError, r"must lie in \[1, pgd_steps - 1\]"),
])
def test_refusals_by_rule_and_message(flags, key, exc, msg):
    from paa_amd import attack_clips
    from paa_amd.training_utils import modes
    a = _args(**{**QIN, **flags})
    m, ctx = modes.Modes.of(a), modes.anneal_ctx(a)
    r = modes.RULES[key]
    assert r.exc is exc and r.when(m, ctx)
    with pytest.raises(exc, match=msg):
        modes.check(m, (key,), ctx)
    assert [k for k in modes.ANNEAL if (modes.RULES[k].mode is None or getattr(m, modes.RULES[k].mode)) and
            modes.RULES[k].when(m, ctx)][0] == key                      # it is the one that wins the walk
    with pytest.MonkeyPatch.context() as mp:                             # the entry point raises it before it asks for a GPU
        import torch
        mp.setattr(torch.cuda, "is_available", lambda: False)
        with pytest.raises(exc, match=msg):
            attack_clips.main(a)


def test_rules_off_and_passing():
    from paa_amd.training_utils import modes
    assert modes.ANNEAL == ("anneal_alpha0", "anneal_range", "anneal_stage", "anneal_route")
    assert modes.RULES["anneal_route"].exc is NotImplementedError and modes.RULES["anneal_route"].mode == "anneal_on"
    # with the schedule off none of the flags is looked at, but --stage1_steps alone is refused
    a = _args(alpha_up=0.5, alpha_min=-1.0)
    modes.check(modes.Modes.of(a), modes.ANNEAL, modes.anneal_ctx(a, wer_why="anything"))
    with pytest.raises(ValueError, match="--stage1_steps applies to the two-stage run"):
        modes.check(modes.Modes.of(_args(stage1_steps=2)), modes.ANNEAL_FLAGS, modes.anneal_ctx(_args(stage1_steps=2)))
    with pytest.raises(ValueError, match="--stage1_steps applies to the two-stage run"):
        a = _args(bound_search="shrink", stage1_steps=2)
        modes.check(modes.Modes.of(a), modes.ANNEAL_FLAGS, modes.anneal_ctx(a))
    # the schedule alone, and the two-stage run with the default and an explicit split, pass
    for kw in ({}, dict(bound_search="shrink", pgd_steps=8), dict(bound_search="shrink", pgd_steps=8, stage1_steps=1),
               dict(bound_search="shrink", pgd_steps=8, stage1_steps=7), dict(bound_search="shrink", pgd_steps=2)):
        a = _args(**QIN, **kw)
        modes.check(modes.Modes.of(a), modes.ANNEAL, modes.anneal_ctx(a))
    assert modes.stage1_of(None, 9) == 4 and modes.stage1_of(3, 9) == 3
    # the masking norm: refused by the search's own rule in the two-stage run, fine with the schedule alone
    a = _args(**{**QIN, "norm_type": "linf+masking"})
    modes.check(modes.Modes.of(a), modes.SEARCH_FLAGS + modes.ANNEAL, modes.anneal_ctx(a))
    a.bound_search = "shrink"
    with pytest.raises(NotImplementedError, match="not implemented with --norm_type masking"):
        modes.check(modes.Modes.of(a), modes.SEARCH_FLAGS + modes.ANNEAL, modes.anneal_ctx(a))


def test_route_refusals_name_the_reason():
    from paa_amd import attack_clips
    from paa_amd.core import loss_helpers
    from paa_amd.training_utils import modes
    a = _args(**QIN)
    m = modes.Modes.of(a)
    for why in ("the vocabulary is not one character per token", f"a reference needs more than {loss_helpers.R_CAP} entries"):
        with pytest.raises(NotImplementedError, match=re.escape("--alpha_search qin decides success from the on-device WER counters, "
                                                                "which are not available: " + why)):
            modes.check(m, ("anneal_route",), modes.anneal_ctx(a, wer_why=why))
    bpe = types.SimpleNamespace(get_vocab=lambda: {"<pad>": 0, "he": 1, "llo": 2, "|": 3}, all_special_ids=[0], word_delimiter_token="|")
    with pytest.raises(NotImplementedError, match="the vocabulary is not one character per token"):
        attack_clips.anneal_route(a, bpe, ["hello"])
    with pytest.raises(NotImplementedError, match=f"a reference needs more than {loss_helpers.R_CAP} entries"):
        attack_clips.anneal_route(a, None, ["a " * (loss_helpers.R_CAP + 1)])
    cfg, canon, refs = attack_clips.anneal_route(a, None, ["hello world", "yes"])
    assert cfg == modes.AnnealConfig.of(a) and tuple(refs.shape) == (2, loss_helpers.R_CAP)
    assert refs[1, :5].tolist() == [ord("y"), ord("e"), ord("s"), 0, -1]


def test_stepper_refusals():
    import torch
    from paa_amd.training_utils import clip_attack, modes
    model = types.SimpleNamespace(device=torch.device("cpu"), max_batch=2, length=16000, lengths_on=False)
    cfg = modes.AnnealConfig(1.2, 0.8, 20, 50, 1e-7, 1e-3, 500, False)
    a = _args(norm_type="linf", masking_loss_alpha=1e-5)
    with pytest.raises(ValueError, match="device_wer=True"):
        clip_attack.ClipStepper(model, a, 16000, anneal=cfg)
    with pytest.raises(ValueError, match="needs --masking_loss_alpha > 0"):
        clip_attack.ClipStepper(model, _args(norm_type="linf"), 16000, device_wer=True, anneal=cfg)
    with pytest.raises(ValueError, match="alpha_up must be finite and > 1"):
        clip_attack.ClipStepper(model, a, 16000, device_wer=True, anneal=cfg._replace(up=0.9))
    with pytest.raises(ValueError, match="the clamps must enclose the starting weight"):
        clip_attack.ClipStepper(model, a, 16000, device_wer=True, anneal=cfg._replace(alpha_min=1e-4))
    with pytest.raises(ValueError, match="one stepper per stage"):
        clip_attack.ClipStepper(model, a, 16000, device_wer=True, anneal=cfg, search=modes.SearchConfig(0.8, 0.01, 500, False))
    assert clip_attack.AnnealConfig is modes.AnnealConfig


def test_masking_loss_refuses_bad_host_alphas():
    import torch
    from paa_amd.core import masking
    dev = torch.device("cpu")
    for bad in ([1.0, -0.5], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError, match="finite and >= 0"):
            masking._alpha_dev(bad, 2, dev)
    with pytest.raises(ValueError, match="one value per clip"):
        masking._alpha_dev([1.0], 2, dev)
    a = masking._alpha_dev(np.array([0.0, 0.5]), 2, dev)
    assert a.dtype == torch.float32 and a.tolist() == [0.0, 0.5]


# ---- records and summary --------------------------------------------------------------------------------------------------------
def _rec(i, **kw):
    return {"index": i, "clean_wer": 0.0, "adv_wer": 0.5 * i, "clean_ctc": 1.0, "final_ctc": 2.0 + i, "l2": 0.1, "linf": 0.01,
            "snr_db": 40.0} | kw


def test_summary_and_results_without_the_fields_are_todays():
    from paa_amd import attack_clips
    recs = [_rec(0), _rec(1), _rec(2)]
    s = attack_clips.summarize(recs)
    assert list(s) == ["clean_wer", "adv_wer", "final_ctc", "l2", "linf", "snr_db", "clips"]
    a = _args(norm_type="snr", pgd_steps=3)
    want = {"norm_type": "snr", "attack_mode": "untargeted", "optimizer_type": a.optimizer_type, "split": "test", "pgd_steps": 3,
            "clips": recs, "summary": s}
    assert json.dumps(attack_clips.results_dict(recs, a), indent=2) == json.dumps(want, indent=2)
    srch = [_rec(0, found=True, found_step=4, bound_scale=0.5, last_scale=0.4)]
    assert list(attack_clips.summarize(srch))[-3:] == ["clips", "success_rate", "mean_bound_scale"]
    assert attack_clips.RECORD_FIELDS == ("index", "clean_wer", "adv_wer", "clean_ctc", "final_ctc", "l2", "linf", "snr_db")
    assert attack_clips.SEARCH_FIELDS == ("found", "found_step", "bound_scale", "last_scale")


def test_summary_with_the_fields():
    from paa_amd import attack_clips
    assert attack_clips.ANNEAL_FIELDS == ("alpha_found", "alpha_step", "best_masking_loss", "best_alpha", "last_alpha")
    assert attack_clips.STAGE1_FIELD == "stage1_masking_loss"
    nan = float("nan")
    recs = [_rec(0, alpha_found=True, alpha_step=4, best_masking_loss=2.0, best_alpha=1e-5, last_alpha=2e-5),
            _rec(1, alpha_found=False, alpha_step=-1, best_masking_loss=nan, best_alpha=1e-6, last_alpha=1e-6),
            _rec(2, alpha_found=True, alpha_step=9, best_masking_loss=1.0, best_alpha=3e-5, last_alpha=3e-5)]
    s = attack_clips.summarize(recs)
    assert list(s)[-3:] == ["clips", "alpha_success_rate", "mean_best_masking_loss"]
    assert s["alpha_success_rate"] == 2 / 3 and s["mean_best_masking_loss"] == 1.5
    none = attack_clips.summarize(recs[1:2])
    assert none["alpha_success_rate"] == 0.0 and np.isnan(none["mean_best_masking_loss"])
    both = [dict(r, found=True, found_step=1, bound_scale=0.5, last_scale=0.4, stage1_masking_loss=3.0) for r in recs]
    s2 = attack_clips.summarize(both)
    assert list(s2)[-5:] == ["clips", "success_rate", "mean_bound_scale", "alpha_success_rate", "mean_best_masking_loss"]
    json.dumps(attack_clips.results_dict(both, _args(**QIN, bound_search="shrink")))


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
        assert name in declared and name in lib.exported_symbols() and hasattr(L, name), name
    assert L.paa_version() in lib.ABI_VERSIONS == (350, 351)
    assert len(lib._SIGS["paa_masking_loss_rows"][1]) == len(lib._SIGS["paa_masking_loss"][1]) + 1
    assert len(lib._SIGS["paa_clip_anneal"][1]) == 20


def test_entries_refuse_bad_arguments_on_the_host(lib):
    """Every refusal comes back before a launch: no GPU is needed to get it."""
    L = lib.lib()
    d = C.c_void_p(64)                      # never dereferenced
    ptrs = ("delta", "counts", "loss", "alpha", "best", "bloss", "balpha", "bstep", "step")
    ok = dict(B=2, L=8, targeted=0, milli=500, up_every=20, down_every=50, up=1.2, down=0.8, lo=1e-7, hi=1e-3, **{k: d for k in ptrs})

    def call(**kw):
        a = {**ok, **kw}
        return L.paa_clip_anneal(a["delta"], a["B"], a["L"], a["counts"], a["loss"], a["targeted"], a["milli"], a["up_every"],
                                 a["down_every"], a["up"], a["down"], a["lo"], a["hi"], a["alpha"], a["best"], a["bloss"], a["balpha"],
                                 a["bstep"], a["step"], None)
    for k in ptrs:
        assert call(**{k: None}) == lib.PAA_ERR_ARG, k
        assert b"paa_clip_anneal: null" in L.paa_last_error()
    inf, nan = float("inf"), float("nan")
    for kw in (dict(B=0), dict(B=65536), dict(L=0), dict(milli=0), dict(up_every=0), dict(down_every=0), dict(up=1.0), dict(up=inf),
               dict(up=nan), dict(down=0.0), dict(down=1.0), dict(down=nan), dict(lo=0.0), dict(lo=nan), dict(lo=2e-3), dict(hi=inf),
               dict(hi=nan)):
        assert call(**kw) == lib.PAA_ERR_ARG, kw
        assert b"paa_clip_anneal" in L.paa_last_error()
    # paa_masking_loss_rows: the null check comes first, as paa_masking_loss's does
    assert L.paa_masking_loss_rows(None, None, None, 2, None, 2, 16000, d, 2, None, None, None, None, None) == lib.PAA_ERR_ARG
    assert b"paa_masking_loss_rows: null" in L.paa_last_error()
    assert L.paa_masking_loss(None, None, None, 2, None, 2, 16000, d, None, None, None, None, None) == lib.PAA_ERR_ARG
    assert b"paa_masking_loss: null" in L.paa_last_error()
