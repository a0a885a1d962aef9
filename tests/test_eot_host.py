"""No-GPU checks of per-clip perturbations through the playback chain: the numpy reference pinned to the
placement layer's, the parser and the mode record, the new rules with their exception types, the refusals that stay when the mode
is off, the sites of a ``ClipChain`` built on the CPU device, the results' new keys, and the three new C-ABI entries (declared,
exported, bound, refusing bad arguments before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eot_ref as ER
import place_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_eot_rows", "paa_eot_reduce", "paa_eot_vote")


def _parse(*argv):
    from paa_amd import attack_clips
    return attack_clips.create_arg_parser().parse_args(list(argv))


def _normal(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


# ---- the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,L", [(1, 1), (5, 257), (8, 1000)])
def test_reference_is_the_placement_layers_at_one_clip(G, L):
    g_rows, gain = _normal(G * L, 1).reshape(G, L), np.exp2(_normal(G, 2)).astype(np.float32)
    for a in (gain, None):
        want = PR.reduce64(g_rows, [0] * G, a, L)[0].astype(np.float32)
        got = ER.reduce64(g_rows, a, G)
        assert got.shape == (1, L) and got.dtype == np.float32 and np.array_equal(got[0].view(np.int32), want.view(np.int32))
    x, d = _normal(L, 3), _normal(L, 4) * np.float32(1e-2)
    for a in (gain, None):
        want = PR.place((x + d).astype(np.float32), L, [0] * G, a)
        got = ER.rows32(x[None], d[None], a, G)
        assert got.shape == (G, L) and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(ER.rows32(None, d[None], None, G), np.repeat(d[None], G, axis=0))
    assert np.array_equal(ER.clean_rows(x[None], G), np.repeat(x[None], G, axis=0))


def test_reference_rows_and_reduce_on_several_clips():
    B, G, L = 3, 4, 50
    x, d, a = _normal(B * L, 5).reshape(B, L), _normal(B * L, 6).reshape(B, L), np.exp2(_normal(B * G, 7)).astype(np.float32)
    rows = ER.rows32(x, d, a, G)
    g = _normal(B * G * L, 8).reshape(B * G, L)
    grad = ER.reduce64(g, a, G)
    for b in range(B):
        for k in range(G):
            assert np.array_equal(rows[b * G + k], a[b * G + k] * (x[b] + d[b]))          # float32 throughout: add, then multiply
        want = sum(float(a[b * G + k]) * g[b * G + k].astype(np.float64) for k in range(G))
        assert np.array_equal(grad[b], want.astype(np.float32))


def test_reference_vote_on_hand_made_triples():
    rows = [[3, 5, 4], [1, 5, 6], [1, 5, 7], [2, 5, 5],          # clip 0: fewest 1 (first at g = 1), most 3 (g = 0)
            [0, 2, 2], [0, 2, 9], [4, 2, 1], [4, 2, 3]]          # clip 1: fewest 0 (tie: g = 0), most 4 (tie: g = 2)
    assert ER.vote(rows, 4, False).tolist() == [[1, 5, 6], [0, 2, 2]]
    assert ER.vote(rows, 4, True).tolist() == [[3, 5, 4], [4, 2, 1]]
    assert ER.vote(rows, 1, False).tolist() == rows == ER.vote(rows, 1, True).tolist()          # one draw: the draw
    assert ER.vote(rows, 2, True).tolist() == [[3, 5, 4], [2, 5, 5], [0, 2, 2], [4, 2, 1]]
    assert ER.vote([[7, 1, 1]] * 3, 3, True).tolist() == [[7, 1, 1]]


# ---- the parser and the mode record ---------------------------------------------------------------------------------------
def test_parser_and_modes():
    from paa_amd.training_utils.modes import Modes
    a = _parse()
    assert a.eot_draws == 0 and a.eot_eval_draws is None
    m = Modes.of(a)
    assert m.eot_draws == 0 and not m.eot_on and not m.seconds_on and not m.link_on
    assert Modes.of().eot_draws == 0 and Modes.__dataclass_fields__["eot_draws"].default == 0
    a = _parse("--eot_draws", "4", "--eot_eval_draws", "16", "--noise_snr_db", "10", "30")
    m = Modes.of(a)
    assert m.eot_draws == 4 and m.eot_on and m.link_on and m.chan_on and not m.place_on and a.eot_eval_draws == 16
    assert Modes.of(a, eot_draws=0).eot_on is False and Modes.of(eot_draws=True).eot_on is False
    assert Modes.of(_parse("--perturbation_seconds", "0.5")).seconds_on


def test_new_rules_and_their_exception_types():
    from paa_amd.training_utils import modes
    from paa_amd.training_utils.modes import Modes, check
    assert modes.EOT == ("eot_range", "eot_links", "eot_shift") and list(modes.RULES)[-3:] == list(modes.EOT)
    for bad in (-1, 65, 2.0, "3", True, None):
        with pytest.raises(ValueError, match=r"eot_draws must be an integer in \[0, 64\]"):
            check(Modes.of(eot_draws=bad) if bad is not None else modes.replace(Modes.of(), eot_draws=None), ("eot_range",))
    for ok in (0, 1, 64):
        check(Modes.of(eot_draws=ok), ("eot_range",))
    with pytest.raises(ValueError, match="at least one link"):
        check(Modes.of(eot_draws=2), modes.EOT)
    check(Modes.of(), modes.EOT)                                         # off: nothing applies
    for link in (dict(place_gain_db=3.0), dict(rir_bank="synthetic"), dict(drift_ppm=500.0), dict(noise_snr_db=[10.0, 30.0])):
        check(Modes.of(eot_draws=2, **link), modes.EOT)
    for shift in (dict(place_shift="random"), dict(perturbation_seconds=0.5), dict(perturbation_seconds=0.5, rir_bank="synthetic")):
        with pytest.raises(NotImplementedError, match="no position of its own"):
            check(Modes.of(eot_draws=2, **shift), modes.EOT)
        check(Modes.of(eot_draws=0, **shift), modes.EOT)


def test_main_with_the_mode_on_raises_the_new_rules_and_the_links_own(monkeypatch):
    """Before any launch, so no GPU is needed: the new rules, then the masking / length refusals of the links that are on."""
    from paa_amd import attack_clips
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="eot_draws must be an integer"):
        attack_clips.main(_parse("--eot_draws", "65", "--place_gain_db", "3"))
    with pytest.raises(ValueError, match="at least one link"):
        attack_clips.main(_parse("--eot_draws", "2"))
    with pytest.raises(NotImplementedError, match="no position of its own"):
        attack_clips.main(_parse("--eot_draws", "2", "--place_shift", "random"))
    with pytest.raises(NotImplementedError, match="masking"):
        attack_clips.main(_parse("--eot_draws", "2", "--place_gain_db", "3", "--norm_type", "masking"))
    with pytest.raises(NotImplementedError, match="masking"):
        attack_clips.main(_parse("--eot_draws", "2", "--drift_ppm", "500", "--norm_type", "linf", "--masking_loss_alpha", "0.5"))
    with pytest.raises(ValueError, match="clip_lengths true does not support"):
        attack_clips.main(_parse("--eot_draws", "2", "--rir_bank", "synthetic", "--clip_lengths", "true"))
    with pytest.raises(ValueError, match="eot_eval_draws"):
        attack_clips.main(_parse("--eot_draws", "2", "--place_gain_db", "3", "--eot_eval_draws", "0"))
    with pytest.raises(SystemExit, match="needs a GPU"):                 # every refusal passed: the next stop is the device
        attack_clips.main(_parse("--eot_draws", "2", "--rir_bank", "synthetic", "--rir_taps", "64", "--noise_snr_db", "20", "30"))


@pytest.mark.parametrize("flags", [("--rir_bank", "synthetic"), ("--drift_ppm", "500"), ("--place_gain_db", "3"),
                                   ("--noise_snr_db", "10", "30"), ("--place_shift", "random")])
def test_off_path_keeps_its_refusals(flags):
    from paa_amd import attack_clips
    for extra in ((), ("--eot_draws", "0")):
        with pytest.raises(NotImplementedError, match="per-clip"):
            attack_clips.main(_parse(*flags, *extra))


# ---- the chain's sites ----------------------------------------------------------------------------------------------------
def test_clip_chain_sites_on_the_cpu():
    from paa_amd.training_utils import chain, place
    dev, L, G, R = torch.device("cpu"), 400, 3, 6
    a = _parse("--norm_type", "linf", "--place_gain_db", "3", "--rir_bank", "synthetic", "--rir_count", "2", "--rir_taps", "16",
               "--drift_ppm", "500", "--noise_snr_db", "10", "30")
    ch = chain.ClipChain(a, dev, R, L, G, place.STREAM_TRAIN, clip_base=12)
    assert isinstance(ch, chain.PlaybackChain) and ch.G == G
    assert ch.placer.max_batch == ch.reverb.max_batch == ch.chan.max_batch == R          # every link sized R = B * G
    assert not ch.placer.shift_on and ch.placer.Lp == L and ch.placer.gain_db == 3.0 and not ch.placer.explicit
    assert ch.clean_rows.shape == (R, L) and ch.placer.grad_rows.shape == (R, L)
    assert ch.clip_base == 12 and all(s.clip_base == 12 for s in (ch.placer, ch.reverb, ch.chan))
    got = ch.counters()
    want = [ch.placer.counter, ch.reverb.counter, ch.chan.counter, ch.chan.noise_counter]
    assert len(got) == 4 and all(g is w for g, w in zip(got, want))
    ch.set_step(9)
    assert [int(c) for c in got] == [9] * 4
    # noise off: no per-row clean copy; gain off: the placer is pinned at gain 1 and draws nothing
    ch = chain.ClipChain(_parse("--norm_type", "linf", "--drift_ppm", "500"), dev, R, L, G, place.STREAM_EVAL, with_grad=False)
    assert ch.clean_rows is None and ch.placer.explicit and ch.reverb is None and ch.placer.grad_rows is None
    assert [c is w for c, w in zip(ch.counters(), [ch.chan.counter, ch.chan.noise_counter])] == [True, True]
    with pytest.raises(ValueError, match="draws per clip"):
        chain.ClipChain(a, dev, 2, L, 3, place.STREAM_TRAIN)
    # one copy of the link order: the per-clip chain defines the two ends and nothing between them
    assert "_links" not in vars(chain.ClipChain) and "_links_back" not in vars(chain.ClipChain)


# ---- the results' new keys ------------------------------------------------------------------------------------------------
def test_results_and_summary_keys():
    from paa_amd import attack_clips
    base = {"index": 0, "clean_wer": 0.0, "adv_wer": 1.0, "clean_ctc": 1.0, "final_ctc": 9.0, "l2": 1.0, "linf": 0.1, "snr_db": 30.0}
    off = _parse("--norm_type", "linf")
    d = attack_clips.results_dict([dict(base)], off)
    assert list(d) == ["norm_type", "attack_mode", "optimizer_type", "split", "pgd_steps", "clips", "summary"]          # today's
    assert not any(k.startswith("eot") for k in d["summary"]) and attack_clips.eot_eval_draws(off) == 0
    on = _parse("--norm_type", "linf", "--eot_draws", "2", "--rir_bank", "synthetic", "--rir_count", "2", "--rir_taps", "16",
                "--noise_snr_db", "20", "30")
    recs = [dict(base, eot_adv_wer=0.5, eot_clean_wer=0.0, eot_success=0.5, eot_draws=2),
            dict(base, index=1, eot_adv_wer=1.0, eot_clean_wer=0.5, eot_success=1.0, eot_draws=2)]
    d = attack_clips.results_dict(recs, on, 8000)
    assert d["eot_draws"] == 2 and d["eot_eval_draws"] == 2 and d["rir_taps"] == 16 and d["noise_snr_db"] == [20.0, 30.0]
    assert d["summary"]["eot_adv_wer"] == 0.75 and d["summary"]["eot_clean_wer"] == 0.25 and d["summary"]["eot_success"] == 0.75
    on.eot_eval_draws = 5
    assert attack_clips.eot_eval_draws(on) == 5
    assert attack_clips.EOT_FIELDS == ("eot_adv_wer", "eot_clean_wer", "eot_success", "eot_draws")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
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
    assert [len(lib._SIGS[n][1]) for n in NEW_ENTRIES] == [9, 7, 6]
    from paa_amd import build_ext
    assert "eot_kernels.hip" in build_ext.SOURCES


def test_entries_refuse_bad_arguments_on_the_host(lib):
    """Every refusal comes back before a launch: no GPU is needed to get it."""
    L, ARG = lib.lib(), lib.PAA_ERR_ARG
    d = C.c_void_p(64)                      # never dereferenced
    for B, G, n in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (-1, 2, 8), (65536, 32768, 8), (2 ** 31 - 1, 2, 8)):
        assert L.paa_eot_rows(d, d, d, d, d, B, G, n, None) == ARG, (B, G, n)
        assert L.paa_eot_reduce(d, d, d, B, G, n, None) == ARG, (B, G, n)
        if n:
            assert L.paa_eot_vote(d, B, G, 0, d, None) == ARG, (B, G)
    assert b"INT32_MAX" in L.paa_last_error()
    assert L.paa_eot_rows(d, None, d, d, d, 2, 2, 8, None) == ARG and L.paa_eot_rows(d, d, d, None, d, 2, 2, 8, None) == ARG
    assert b"null" in L.paa_last_error()
    assert L.paa_eot_rows(None, d, d, d, d, 2, 2, 8, None) == ARG          # a per-row clean copy needs the clean batch
    assert b"d_clean_rows needs d_clean" in L.paa_last_error()
    assert L.paa_eot_reduce(None, d, d, 2, 2, 8, None) == ARG and L.paa_eot_reduce(d, d, None, 2, 2, 8, None) == ARG
    assert L.paa_eot_vote(None, 2, 2, 0, d, None) == ARG and L.paa_eot_vote(d, 2, 2, 1, None, None) == ARG
