"""CPU: temporal masking of the masking threshold: the decrement tables, the reference spread
(tests/mask_time_ref.py) and its invariants, the burst clip, and the host plumbing (parser, mode rules, run naming, ABI entry)."""
import os
import re
import types

import numpy as np
import pytest

import mask_time_ref as MT
import masking_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


# ------------------------------------------------------------------------------------------------ tables
def test_table_values():
    post, pre = MT.tables(200.0, 20.0)
    assert post.dtype == pre.dtype == np.float32 and len(post) == 19 and len(pre) == 1
    assert MT.lags(200.0) == 19 and MT.lags(20.0) == 1 and MT.lags(0.0) == 0
    np.testing.assert_array_equal(post, (4.8 * np.arange(1, 20)).astype(np.float32))
    np.testing.assert_array_equal(pre, np.float32([48.0]))
    # the boundary: at P = 200 ms lag 20 would be exactly 96 dB, which is not under the range
    assert 20 * 60.0 * 256 * 1000.0 == 96.0 * 200.0 * 16000 and 20 * 4.8 == 96.0
    assert MT.lags(200.0 + 1e-9) == 20 and MT.lags(200.0 - 1e-9) == 19
    assert MT.lags(320.0) == 31 and MT.lags(330.0) == 32 and MT.lags(330.0 + 1e-6) == 33 and MT.lags(10.0) == 0
    assert (np.diff(post) > 0).all() and post[-1] < 96.0


def test_package_tables_equal_the_reference():
    from paa_amd.core.masking import temporal_tables
    from paa_amd.training_utils import modes
    for post_ms, pre_ms, hop, sr in ((200.0, 20.0, 256, 16000), (320.0, 0.0, 256, 16000), (0.0, 20.0, 256, 16000),
                                     (330.0, 10.5, 256, 16000), (100.0, 30.0, 128, 8000), (150.0, 12.0, 256, 22050)):
        a = types.SimpleNamespace(masking_post_ms=post_ms, masking_pre_ms=pre_ms, hop_length=hop, sr=sr)
        got, want = temporal_tables(a), MT.tables(post_ms, pre_ms, hop, sr)
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and np.array_equal(g, w), (post_ms, pre_ms, hop, sr)
        assert modes.mask_time_lags(post_ms, hop, sr) == len(want[0])
    post, pre = temporal_tables(types.SimpleNamespace())             # an args object without the flags
    assert post.dtype == pre.dtype == np.float32 and post.shape == pre.shape == (0,)


# ------------------------------------------------------------------------------------------------ the reference spread
def _theta(T=40, F=9, seed=1, holes=True):
    rng = np.random.default_rng(seed)
    th = (rng.standard_normal((T, F)) * 25.0 + 30.0).astype(np.float32)
    if holes:
        th[rng.random((T, F)) < 0.3] = NINF
        th[:, 0] = NINF
    return th


def test_reference_properties():
    post, pre = MT.tables(200.0, 20.0)
    th = _theta()
    sp = MT.spread32(th, post, pre)
    assert sp.dtype == np.float32 and sp.shape == th.shape
    assert (sp >= th).all() and (sp > th).any()
    assert np.isneginf(sp[:, 0]).all()                                # nothing reaches the column: -inf stays -inf
    const = np.broadcast_to(_theta(1, 9, 2, holes=False), (40, 9)).copy()
    assert np.array_equal(MT.spread32(const, post, pre), const)       # constant in time: unchanged
    none = np.zeros(0, np.float32)
    assert np.array_equal(MT.spread32(th, none, none), th)            # both tables empty: the identity
    assert np.array_equal(MT.spread64(th, none, none), th.astype(np.float64))
    # a batch axis spreads every clip on its own
    two = np.stack([th, _theta(seed=5)])
    assert np.array_equal(MT.spread32(two, post, pre)[1], MT.spread32(two[1], post, pre))


@pytest.mark.parametrize("T,t0", [(40, 25), (40, 0), (40, 39), (3, 1), (2, 0), (1, 0)])
def test_impulse_response_is_the_tables(T, t0):
    post, pre = MT.tables(320.0, 40.0)                                # J = 31 and 3: longer than the short T
    assert len(post) == 31 and len(pre) == 3
    th = np.full((T, 2), NINF, np.float32)
    th[t0, 1] = 50.0
    sp = MT.spread32(th, post, pre)
    want = np.full(T, NINF, np.float32)
    want[t0] = 50.0
    for j in range(1, 32):
        if t0 + j < T:
            want[t0 + j] = np.float32(50.0) - post[j - 1]
    for j in range(1, 4):
        if t0 - j >= 0:
            want[t0 - j] = np.float32(50.0) - pre[j - 1]
    assert np.array_equal(sp[:, 1], want) and np.isneginf(sp[:, 0]).all()


def test_spread32_against_spread64():
    for post_ms, pre_ms in ((200.0, 20.0), (320.0, 0.0), (0.0, 20.0), (123.0, 17.0)):
        post, pre = MT.tables(post_ms, pre_ms)
        th = _theta(T=60, F=33, seed=3)
        s32, s64 = MT.spread32(th, post, pre).astype(np.float64), MT.spread64(th, post, pre)
        both_inf = np.isneginf(s32) & np.isneginf(s64)
        assert (np.isneginf(s32) == np.isneginf(s64)).all()
        err = np.where(both_inf, 0.0, np.abs(np.where(both_inf, 0.0, s32) - np.where(both_inf, 0.0, s64)))
        # one f32 subtraction per term: half an ulp of the result, and the maximum is exact; one ulp of the larger operand bounds it
        ulp = np.spacing(np.maximum(np.abs(np.where(both_inf, 1.0, s64)), 96.0).astype(np.float32)).astype(np.float64)
        assert (err <= ulp).all(), (post_ms, pre_ms, (err / ulp).max())


# ------------------------------------------------------------------------------------------------ the burst clip
def test_burst_clip():
    """Post-masking fills the silence after the burst, pre-masking the frame before it.  At bin 64 (1 kHz) the frames after the burst
    follow the loudest decayed frame: frame 32 (85.25 dB) stands 13.95 dB above frame 33 (71.30 dB), more than one 4.8 dB step, so
    by the definition theta'(33 + j) = theta(32) - 4.8 (j + 1) for j = 1..18 (not theta(33) - 4.8 j, which lies 9.15 dB lower), and
    frame 52 is out of frame 32's window (lag 20 > J = 19) while theta(33) - 91.2 is under the threshold in quiet: it keeps it."""
    pbar, theta, pmax = MR.threshold(MT.burst_clip())
    assert theta.shape == (63, 513)
    assert np.allclose(theta[34:63, 64], -8.6309, atol=1e-3)                  # the threshold in quiet after the burst
    assert (theta[16:33, 64] > 85.0).all() and (theta[16:33, 64] < 89.5).all()
    post, pre = MT.tables(200.0, 20.0)
    th = theta.astype(np.float32)
    sp = MT.spread32(th, post, pre)
    rose = sp > th
    assert sorted(set(np.nonzero(rose.any(axis=1))[0].tolist())) == [14] + list(range(32, 53))
    assert np.array_equal(sp[:14], th[:14]) and np.array_equal(sp[53:], th[53:])          # frames 0-13 and 53-62: untouched
    assert rose.mean() == pytest.approx(0.157, abs=1e-3)
    up = np.where(rose, sp.astype(np.float64) - np.where(np.isneginf(th), np.nan, th), 0.0)
    assert 80.0 < np.nanmax(up) < 96.0                                        # by up to 84 dB
    s64 = MT.spread64(theta, post, pre)
    for j in range(1, 19):
        assert s64[33 + j, 64] == pytest.approx(theta[32, 64] - 4.8 * (j + 1), abs=1e-5), j
        assert float(sp[33 + j, 64]) == pytest.approx(s64[33 + j, 64], abs=1e-5)
        assert s64[33 + j, 64] >= theta[33, 64] - 4.8 * j                     # never under the chain from frame 33
    assert np.allclose(np.diff(s64[34:52, 64]), -4.8, atol=1e-5)              # 4.8 dB per frame
    assert s64[52, 64] == theta[52, 64] and theta[33, 64] - 4.8 * 19 < theta[52, 64]
    assert s64[14, 64] == pytest.approx(theta[15, 64] - 48.0, abs=1e-9)        # pre-masking: one frame, 48 dB down


def test_speech_like_clips_rise_by_a_few_percent():
    from paa_amd import synth
    x = synth.clean_audio(2, 16000)
    share = []
    for b in range(2):
        th = MR.threshold(x[b])[1].astype(np.float32)
        share.append(float((MT.spread32(th, *MT.tables(200.0, 20.0)) > th).mean()))
    assert share[0] == pytest.approx(0.052, abs=2e-3) and share[1] == pytest.approx(0.063, abs=2e-3)


# ------------------------------------------------------------------------------------------------ host plumbing
def test_parser_defaults():
    from paa_amd import attack_clips
    from paa_amd.training_utils import parser
    for make in (parser.create_arg_parser, attack_clips.create_arg_parser):
        a = make().parse_args([])
        assert a.masking_post_ms == 0.0 and a.masking_pre_ms == 0.0
        a = make().parse_args(["--norm_type", "masking", "--masking_post_ms", "200", "--masking_pre_ms", "20"])
        assert a.masking_post_ms == 200.0 and a.masking_pre_ms == 20.0


def _ns(**kw):
    return types.SimpleNamespace(**{"norm_type": "masking", "hop_length": 256, "sr": 16000, **kw})


def test_mode_rules():
    from paa_amd.training_utils import modes
    from paa_amd.training_utils.modes import MASK_TIME, RULES, Modes, check
    assert MASK_TIME == ("mask_time_range", "mask_time_unused")
    assert RULES["mask_time_range"].exc is ValueError and RULES["mask_time_unused"].exc is ValueError
    m = Modes.of()
    assert m.post_ms == 0.0 and m.pre_ms == 0.0 and not m.mask_time_on
    check(m, MASK_TIME)
    for flag in ("masking_post_ms", "masking_pre_ms"):
        check(Modes.of(_ns(**{flag: 200.0})), MASK_TIME)
        check(Modes.of(_ns(**{flag: 330.0})), MASK_TIME)                  # J = 32: the last admissible
        check(Modes.of(_ns(**{flag: 10.001})), MASK_TIME)                 # J = 1
        for bad in (-1.0, float("nan"), float("inf"), 10.0, 5.0, 330.001, 1e6):          # J = 0 at 10 ms; J = 33 past 330 ms
            with pytest.raises(ValueError, match=flag) as e:
                check(Modes.of(_ns(**{flag: bad})), MASK_TIME)
            assert "(10, 330]" in str(e.value) and "256" in str(e.value) and "16000" in str(e.value)
    with pytest.raises(ValueError, match=r"\(5, 165\]"):                  # the range follows the run's hop and sample rate
        check(Modes.of(_ns(masking_post_ms=200.0, hop_length=128)), MASK_TIME)
    check(Modes.of(_ns(masking_post_ms=100.0, hop_length=128)), MASK_TIME)
    # a time without a consumer of the threshold
    with pytest.raises(ValueError, match="masking_post_ms"):
        check(Modes.of(_ns(norm_type="linf", masking_post_ms=200.0)), MASK_TIME)
    with pytest.raises(ValueError, match="masking_loss_alpha"):
        check(Modes.of(_ns(norm_type="linf", masking_pre_ms=20.0, masking_loss_alpha=0.0)), MASK_TIME)
    check(Modes.of(_ns(norm_type="linf", masking_post_ms=200.0, masking_loss_alpha=1e-6)), MASK_TIME)
    check(Modes.of(_ns(norm_type="masking+l2", masking_pre_ms=20.0)), MASK_TIME)
    check(Modes.of(_ns(norm_type="linf")), MASK_TIME)
    # the range wins over the missing consumer
    with pytest.raises(ValueError, match="330"):
        check(Modes.of(_ns(norm_type="linf", masking_post_ms=-3.0)), MASK_TIME)
    # the position constraints of the earlier modes still hold, and the earlier masking refusals are in force with the mode on
    assert list(RULES)[-3:] == list(modes.EOT) and list(Modes.__dataclass_fields__)[-1] == "search_on"
    on = dict(masking_post_ms=200.0, masking_pre_ms=20.0)
    with pytest.raises(NotImplementedError):
        check(Modes.of(_ns(**on)), ("route",), modes.Ctx(2))
    with pytest.raises(ValueError):
        check(Modes.of(_ns(clip_lengths="true", **on)), modes.LENGTHS)
    with pytest.raises(NotImplementedError):
        check(Modes.of(_ns(rir_bank="synthetic", **on)), modes.ROOMS)
    with pytest.raises(NotImplementedError):
        check(Modes.of(_ns(drift_ppm=10.0, **on)), modes.CHANNEL_FLAGS)
    with pytest.raises(NotImplementedError):
        check(Modes.of(_ns(place_shift="random", **on)), modes.PLACE_FLAGS)
    with pytest.raises(NotImplementedError):
        check(Modes.of(_ns(bound_search="shrink", **on)), ("search_masking",))


def test_run_naming_and_result_keys():
    from paa_amd.training_utils import build
    off = _ns()
    assert build.masking_time_suffix(off) == "" and build.masking_time_extra(off) == {}
    assert build.masking_time_suffix(types.SimpleNamespace()) == ""
    on = _ns(masking_post_ms=200.0, masking_pre_ms=20.0)
    assert build.masking_time_suffix(on) == "_mt200-20"
    assert build.masking_time_extra(on) == {"masking_post_ms": 200.0, "masking_pre_ms": 20.0}
    assert build.masking_time_suffix(_ns(masking_post_ms=0.0, masking_pre_ms=12.5)) == "_mt0-12.5"


def test_results_dict_keys_only_with_the_mode_on():
    from paa_amd import attack_clips
    base = dict(norm_type="masking", attack_mode="untargeted", optimizer_type="pgd", split="test", pgd_steps=3, hop_length=256, sr=16000)
    recs = [{"index": 0} | {k: 0.5 for k in attack_clips.SUMMARY_FIELDS}]
    off = attack_clips.results_dict(recs, types.SimpleNamespace(**base))
    on = attack_clips.results_dict(recs, types.SimpleNamespace(**base, masking_post_ms=200.0, masking_pre_ms=20.0))
    assert not [k for k in off if "_ms" in k]
    assert on["masking_post_ms"] == 200.0 and on["masking_pre_ms"] == 20.0
    assert {k: v for k, v in on.items() if "_ms" not in k} == off and list(off) == [k for k in on if "_ms" not in k]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from paa_amd import _lib
    return _lib


def test_entry_declared_exported_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "paa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(paa_[a-z0-9_]+)\s*\(", hdr))
    L = lib.lib()
    name = "paa_proj_set_masking_spread"
    assert name in declared and name in lib.exported_symbols() and hasattr(L, name)
    assert len(lib._SIGS[name][1]) == 5
    assert L.paa_version() in lib.ABI_VERSIONS == (350, 351)
    assert [f[0] for f in lib.PaaParams._fields_][-1] == "masking_margin_db"          # paa_params is untouched
    tab = np.float32([4.8])
    assert L.paa_proj_set_masking_spread(None, 1, tab.ctypes.data, 0, None) == lib.PAA_ERR_ARG      # a null handle: before anything else
