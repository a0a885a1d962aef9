"""No-GPU checks of the per-clip bound search: the numpy statement of the decide / keep / shrink rule against
hand-written cases, the new refusals by rule key and message, the mode record and the flags, the records and the summary with and
without the new fields, and the two new C-ABI entries (declared, exported, bound, refusing bad arguments before any launch)."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

import search_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_project_rows_scaled", "paa_clip_search")


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def test_success_hand_cases():
    # (errors, reference words, hypothesis words)
    counts = [(0, 0, 0),      # e = 0, w = 0: an empty reference is never a success, in either mode
              (3, 0, 3),      # w = 0 untargeted: no reference words, no WER
              (1, 2, 2),      # the exact threshold at wer_milli = 500: 1 * 1000 == 500 * 2
              (499, 1000, 9),  # one error below the threshold of 1000 words: 499000 < 500000
              (500, 1000, 9),  # ... and exactly on it
              (0, 4, 4),      # the transcript exactly
              (7, 4, 11)]     # WER above 1
    assert SR.success(counts, False, 500).tolist() == [False, False, True, False, True, False, True]
    assert SR.success(counts, True, 500).tolist() == [False, False, False, False, False, True, False]
    # thousandths: 0.333 of 3 words needs 0.999 errors, i.e. one
    assert SR.success([(1, 3, 3), (0, 3, 3)], False, 333).tolist() == [True, False]
    assert SR.success([(1, 3, 3)], False, 334).tolist() == [False]
    # the products are taken in 64 bits: the largest counters paa_wer_counts can write and a large threshold do not wrap
    assert SR.success([(8192, 8192, 1)], False, 1000).tolist() == [True]
    assert SR.success([(2 ** 21, 2 ** 21 + 1, 1)], False, 1000).tolist() == [False]


def test_shrink_is_float32_and_reaches_the_floor():
    f = np.float32
    s = SR.shrink_scale([1.0], 0.8, 0.01)
    assert s.dtype == np.float32 and s[0] == f(1.0) * f(0.8) == f(0.8)
    s2 = SR.shrink_scale(s, 0.8, 0.01)
    assert s2[0] == f(f(0.8) * f(0.8)) and s2[0] != np.float64(0.8) * np.float64(0.8)       # rounded after every product
    assert SR.shrink_scale([0.012], 0.8, 0.01)[0] == f(0.01)                                 # 0.0096 < floor
    assert SR.shrink_scale([0.01], 0.8, 0.01)[0] == f(0.01)                                  # stays on the floor
    s = np.array([1.0], dtype=np.float32)
    for _ in range(30):
        s = SR.shrink_scale(s, 0.8, 0.01)
    assert s[0] == f(0.01)
    assert SR.shrink_scale([1.0], 0.5, 1.0)[0] == f(1.0)                                     # floor 1: the scale never moves


def test_clip_search_keeps_only_successes():
    B, L = 4, 5
    delta = np.arange(B * L, dtype=np.float32).reshape(B, L)
    best = np.full((B, L), -7.0, dtype=np.float32)
    scale = np.array([1.0, 0.5, 0.25, 0.011], dtype=np.float32)
    bs = np.array([9.0, 9.0, 9.0, 9.0], dtype=np.float32)
    bstep = np.array([-1, -1, 3, -1], dtype=np.int32)
    counts = [(2, 2, 2), (0, 2, 2), (1, 2, 2), (5, 2, 2)]
    sc, be, bsc, bst, step = SR.clip_search(delta, counts, False, 500, 0.8, 0.01, scale, best, bs, bstep, 6)
    assert step == 7
    assert bst.tolist() == [6, -1, 6, 6] and bsc.tolist() == [1.0, 9.0, 0.25, np.float32(0.011)]
    assert sc.tolist() == [np.float32(0.8), 0.5, np.float32(0.25) * np.float32(0.8), np.float32(0.01)]
    assert np.array_equal(be[[0, 2, 3]], delta[[0, 2, 3]]) and np.all(be[1] == -7.0)
    assert scale[0] == 1.0 and np.all(best == -7.0) and bstep[0] == -1                       # the inputs are left alone
    sc, be, bsc, bst, step = SR.clip_search(delta, counts, True, 500, 0.8, 0.01, scale, best, bs, bstep, 0)
    assert bst.tolist() == [-1, 0, 3, -1] and np.array_equal(be[1], delta[1]) and np.all(be[[0, 2, 3]] == -7.0)


# ---- modes, refusals, flags -----------------------------------------------------------------------------------------------------
def _args(**kw):
    from paa_amd import attack_clips
    a = attack_clips.create_arg_parser().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_flags_and_defaults():
    from paa_amd import attack_clips
    from paa_amd.training_utils import parser
    a = attack_clips.create_arg_parser().parse_args([])
    assert (a.bound_search, a.search_shrink, a.search_floor, a.search_success_wer) == ("off", 0.8, 0.01, 0.5)
    a = attack_clips.create_arg_parser().parse_args(["--bound_search", "shrink", "--search_shrink", "0.5", "--search_floor", "0.1",
                                                     "--search_success_wer", "0.25"])
    assert (a.bound_search, a.search_shrink, a.search_floor, a.search_success_wer) == ("shrink", 0.5, 0.1, 0.25)
    with pytest.raises(SystemExit):
        attack_clips.create_arg_parser().parse_args(["--bound_search", "grow"])
    # the universal runner does not get the flags
    u = parser.create_arg_parser().parse_args([])
    assert not any(hasattr(u, k) for k in ("bound_search", "search_shrink", "search_floor", "search_success_wer"))
    with pytest.raises(SystemExit):
        parser.create_arg_parser().parse_args(["--bound_search", "shrink"])


def test_modes_record_without_the_flags_is_todays():
    from paa_amd.training_utils.modes import Modes
    ns = types.SimpleNamespace(norm_type="snr+linf", masking_loss_alpha=0.0, clip_lengths="true", device_wer=True,
                               optimizer_type="adam")
    m = Modes.of(ns)
    today = Modes(("snr", "linf"), False, 0.0, False, "none", 0.0, False, True, True, "adam")          # the ten fields, in order
    assert m == today and m.search_on is False
    assert list(Modes.__dataclass_fields__)[-1] == "search_on"
    assert Modes.of(_args()).search_on is False
    assert Modes.of(_args(bound_search="shrink")).search_on is True
    assert Modes.of(ns, bound_search="shrink").search_on is True


def test_search_config_of_flags():
    from paa_amd.training_utils.modes import SearchConfig
    assert SearchConfig.of(_args()) is None
    c = SearchConfig.of(_args(bound_search="shrink"))
    assert (c.shrink, c.floor_scale, c.wer_milli, c.targeted) == (0.8, 0.01, 500, False) and c.bad() is None
    c = SearchConfig.of(_args(bound_search="shrink", search_success_wer=0.3336, attack_mode="targeted"))
    assert c.wer_milli == 334 and c.targeted is True


@pytest.mark.parametrize("flags,key,exc,msg", [
    (dict(search_shrink=1.0), "search_range", ValueError, r"search_shrink must lie in \(0, 1\), got 1.0"),
    (dict(search_shrink=0.0), "search_range", ValueError, r"search_shrink must lie in \(0, 1\), got 0.0"),
    (dict(search_shrink=float("nan")), "search_range", ValueError, r"search_shrink must lie in \(0, 1\), got nan"),
    (dict(search_floor=0.0), "search_range", ValueError, r"search_floor must lie in \(0, 1\], got 0.0"),
    (dict(search_floor=1.5), "search_range", ValueError, r"search_floor must lie in \(0, 1\], got 1.5"),
    (dict(search_success_wer=0.0004), "search_range", ValueError, "search_success_wer must be at least 0.0005"),
    (dict(search_success_wer=-1.0), "search_range", ValueError, "search_success_wer must be at least 0.0005"),
    (dict(norm_type="masking"), "search_masking", NotImplementedError, "not implemented with --norm_type masking"),
    (dict(norm_type="snr+masking"), "search_masking", NotImplementedError, "not implemented with --norm_type masking"),
    (dict(norm_type="min_max_freqs"), "search_no_size", ValueError, r"needs a norm with a size to shrink; \('min_max_freqs',\) has none"),
])
def test_refusals_by_rule_and_message(flags, key, exc, msg):
    from paa_amd import attack_clips
    from paa_amd.training_utils import modes
    a = _args(**{"bound_search": "shrink", "norm_type": "snr", **flags})
    m, ctx = modes.Modes.of(a), modes.Ctx(search=modes.SearchConfig.of(a))
    r = modes.RULES[key]
    assert r.mode == "search_on" and r.exc is exc and r.when(m, ctx)
    with pytest.raises(exc, match=msg):
        modes.check(m, (key,), ctx)
    assert [k for k in modes.SEARCH if modes.RULES[k].when(m, ctx)][0] == key          # it is the one that wins the walk
    # the entry point raises it before it asks for a GPU (main leaves with SystemExit right after its refusals otherwise)
    with pytest.MonkeyPatch.context() as mp:
        import torch
        mp.setattr(torch.cuda, "is_available", lambda: False)
        with pytest.raises(exc, match=msg):
            attack_clips.main(a)
    # with the search off none of this is looked at
    a.bound_search = "off"
    modes.check(modes.Modes.of(a), modes.SEARCH, modes.Ctx(search=modes.SearchConfig.of(a), wer_why="anything"))


def test_a_composite_with_one_sized_norm_passes():
    from paa_amd.training_utils import modes
    a = _args(bound_search="shrink", norm_type="min_max_freqs+tv")
    modes.check(modes.Modes.of(a), modes.SEARCH, modes.Ctx(search=modes.SearchConfig.of(a)))


def test_route_refusals_name_the_reason():
    import torch
    from paa_amd import attack_clips
    from paa_amd.core import loss_helpers
    from paa_amd.training_utils import modes
    a = _args(bound_search="shrink", norm_type="snr")
    m, cfg = modes.Modes.of(a), modes.SearchConfig.of(a)
    for why in ("the vocabulary is not one character per token", "a wer_metric object is given",
                f"a reference needs more than {loss_helpers.R_CAP} entries"):
        with pytest.raises(NotImplementedError, match=re.escape("the on-device WER counters, which are not available: " + why)):
            modes.check(m, ("search_route",), modes.Ctx(search=cfg, wer_why=why))
    modes.check(m, ("search_route",), modes.Ctx(search=cfg))
    # attack_clips.search_route finds the reasons itself: a multi-character vocabulary, a reference over the row cap
    bpe = types.SimpleNamespace(get_vocab=lambda: {"<pad>": 0, "he": 1, "llo": 2, "|": 3}, all_special_ids=[0], word_delimiter_token="|")
    with pytest.raises(NotImplementedError, match="the vocabulary is not one character per token"):
        attack_clips.search_route(a, bpe, ["hello"])
    with pytest.raises(NotImplementedError, match=f"a reference needs more than {loss_helpers.R_CAP} entries"):
        attack_clips.search_route(a, None, ["a " * (loss_helpers.R_CAP + 1)])
    cfg2, canon, refs = attack_clips.search_route(a, None, ["hello world", "yes"])
    assert cfg2 == cfg and canon.dtype == torch.int32 and tuple(refs.shape) == (2, loss_helpers.R_CAP)
    assert refs[1, :5].tolist() == [ord("y"), ord("e"), ord("s"), 0, -1]
    # targeted: every clip is judged against the target transcript
    t = _args(bound_search="shrink", norm_type="snr", attack_mode="targeted", target="delete", target_reps=2)
    _, _, refs = attack_clips.search_route(t, None, ["hello world", "yes"])
    want = [ord(ch) for ch in "delete"] + [0]
    assert refs[0, :14].tolist() == want * 2 and refs[1, :15].tolist() == want * 2 + [-1]


def test_stepper_needs_device_wer():
    import torch
    from paa_amd.training_utils import clip_attack, modes
    model = types.SimpleNamespace(device=torch.device("cpu"), max_batch=2, length=16000, lengths_on=False)
    cfg = modes.SearchConfig(0.8, 0.01, 500, False)
    with pytest.raises(ValueError, match="device_wer=True"):
        clip_attack.ClipStepper(model, _args(norm_type="snr"), 16000, search=cfg)
    with pytest.raises(ValueError, match=r"search_shrink must lie in \(0, 1\)"):
        clip_attack.ClipStepper(model, _args(norm_type="snr"), 16000, device_wer=True, search=cfg._replace(shrink=2.0))
    with pytest.raises(NotImplementedError, match="masking"):
        clip_attack.ClipStepper(model, _args(norm_type="masking"), 16000, device_wer=True, search=cfg)
    with pytest.raises(ValueError, match="has none"):
        clip_attack.ClipStepper(model, _args(norm_type="min_max_freqs"), 16000, device_wer=True, search=cfg)


def test_project_rows_refuses_bad_host_scales():
    import torch
    from paa_amd.training_utils import clip_attack
    dev = torch.device("cpu")
    for bad in ([1.0, 0.0], [1.0, -0.5], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError, match="finite and > 0"):
            clip_attack._scale_dev(bad, 2, dev)
    with pytest.raises(ValueError, match="one value per row"):
        clip_attack._scale_dev([1.0], 2, dev)
    s = clip_attack._scale_dev(np.array([1.0, 0.5]), 2, dev)
    assert s.dtype == torch.float32 and s.tolist() == [1.0, 0.5]


# ---- records and summary --------------------------------------------------------------------------------------------------------
def _rec(i, **kw):
    return {"index": i, "clean_wer": 0.0, "adv_wer": 0.5 * i, "clean_ctc": 1.0, "final_ctc": 2.0 + i, "l2": 0.1, "linf": 0.01,
            "snr_db": 40.0} | kw


def test_summary_and_results_without_the_fields_are_todays():
    from paa_amd import attack_clips
    recs = [_rec(0), _rec(1), _rec(2)]
    s = attack_clips.summarize(recs)
    assert list(s) == ["clean_wer", "adv_wer", "final_ctc", "l2", "linf", "snr_db", "clips"]
    assert s["adv_wer"] == 0.5 and s["clips"] == 3
    a = _args(norm_type="snr", pgd_steps=3)
    d = attack_clips.results_dict(recs, a)
    want = {"norm_type": "snr", "attack_mode": "untargeted", "optimizer_type": a.optimizer_type, "split": "test", "pgd_steps": 3,
            "clips": recs, "summary": s}
    assert json.dumps(d, indent=2) == json.dumps(want, indent=2)
    st = attack_clips.summarize([_rec(0, target_wer=1.0)], targeted=True)
    assert list(st)[-2:] == ["target_wer", "clips"]
    assert attack_clips.summarize([])["clips"] == 0


def test_summary_with_the_fields():
    from paa_amd import attack_clips
    assert attack_clips.SEARCH_FIELDS == ("found", "found_step", "bound_scale", "last_scale")
    recs = [_rec(0, found=True, found_step=4, bound_scale=0.5, last_scale=0.4),
            _rec(1, found=False, found_step=-1, bound_scale=1.0, last_scale=1.0),
            _rec(2, found=True, found_step=9, bound_scale=0.25, last_scale=0.2),
            _rec(3, found=False, found_step=-1, bound_scale=1.0, last_scale=1.0)]
    s = attack_clips.summarize(recs)
    assert list(s)[-3:] == ["clips", "success_rate", "mean_bound_scale"]
    assert s["success_rate"] == 0.5 and s["mean_bound_scale"] == 0.375
    none = attack_clips.summarize(recs[1::2])
    assert none["success_rate"] == 0.0 and np.isnan(none["mean_bound_scale"])
    d = attack_clips.results_dict(recs, _args(norm_type="snr", bound_search="shrink"))
    assert d["summary"] == s and all(k in d["clips"][0] for k in attack_clips.SEARCH_FIELDS)
    json.dumps(d)


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
    assert len(lib._SIGS["paa_project_rows_scaled"][1]) == len(lib._SIGS["paa_project_rows"][1]) + 1
    assert len(lib._SIGS["paa_clip_search"][1]) == 14


def test_entries_refuse_bad_arguments_on_the_host(lib):
    """Every refusal comes back before a launch: no GPU is needed to get it."""
    from paa_amd import runtime
    L = lib.lib()
    d = C.c_void_p(64)                      # never dereferenced
    ok = dict(delta=d, B=2, L=8, counts=d, targeted=0, milli=500, shrink=0.8, floor=0.01, scale=d, best=d, bscale=d, bstep=d, step=d)

    def call(**kw):
        a = {**ok, **kw}
        return L.paa_clip_search(a["delta"], a["B"], a["L"], a["counts"], a["targeted"], a["milli"], a["shrink"], a["floor"],
                                 a["scale"], a["best"], a["bscale"], a["bstep"], a["step"], None)
    for k in ("delta", "counts", "scale", "best", "bscale", "bstep", "step"):
        assert call(**{k: None}) == lib.PAA_ERR_ARG, k
        assert b"null" in L.paa_last_error()
    for kw in (dict(B=0), dict(L=0), dict(shrink=0.0), dict(shrink=1.0), dict(shrink=float("nan")), dict(floor=0.0), dict(floor=1.5),
               dict(floor=float("nan")), dict(milli=0), dict(B=65536)):
        assert call(**kw) == lib.PAA_ERR_ARG, kw
    args = _args(norm_type="snr")
    prm = runtime.params_of(args)
    assert L.paa_project_rows_scaled(None, C.byref(prm), None, None, 2, None, 16000, d, None) == lib.PAA_ERR_ARG
    assert L.paa_project_rows_scaled(None, C.byref(prm), None, None, 2, None, 16000, None, None) == lib.PAA_ERR_ARG
