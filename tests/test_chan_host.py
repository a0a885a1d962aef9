"""No-GPU checks of the playback channel: the reference statements of tests/chan_ref.py against a dense
matrix built from the definition, the draw against hand-computed Philox words, the disjointness of the Philox streams, the float32
weight formula against float64, the reference noise, the flags, the refusals at every entry point, and the ABI declarations."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import chan_ref as CR
import place_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_chan_draw", "paa_drift_apply", "paa_noise_add")
ONE = 1 << 32


def _dense(rq, L):
    """The (L, L) float64 matrix of the operator, written from the definition alone: numpy's sinc, no sign identity."""
    A = np.zeros((L, L))
    for i in range(L):
        pos = i * CR.clamp_rq(rq)
        n, f = pos >> 32, (pos & 0xFFFFFFFF) / 2.0 ** 32
        for t in range(-CR.T + 1, CR.T + 1):
            u = t - f
            if 0 <= n + t < L and abs(u) < CR.T:
                A[i, n + t] += np.sinc(u) * 0.5 * (1.0 + np.cos(np.pi * u / CR.T))
    return A


@pytest.mark.parametrize("r", [0.9, 1.0, 1.1])
@pytest.mark.parametrize("L", [5, 16, 257])
def test_references_vs_dense_matrix(L, r):
    rq = CR.rq_of(r)
    rng = np.random.default_rng(L)
    x, g = rng.standard_normal((2, L)), rng.standard_normal((2, L))
    A = _dense(rq, L)
    np.testing.assert_allclose(CR.apply64([rq, rq], x), x @ A.T, rtol=0, atol=1e-13)
    np.testing.assert_allclose(CR.adjoint64([rq, rq], g), g @ A, rtol=0, atol=1e-13)
    # the bound's sums are the same matrix in magnitudes
    want = 2.0 ** -24 * (16.0 * np.abs(x) @ np.abs(A).T + 8.0 * np.abs(x) @ _window(rq, L).T) + 2.0 ** -149
    np.testing.assert_allclose(CR.bound([rq, rq], x), want, rtol=1e-12)


def _window(rq, L):
    W = np.zeros((L, L))
    for i in range(L):
        n = (i * rq) >> 32
        for t in range(-CR.T + 1, CR.T + 1):
            if 0 <= n + t < L:
                W[i, n + t] = 1.0
    return W


def test_unit_ratio_is_the_identity_exactly():
    x = np.random.default_rng(0).standard_normal((3, 300))
    assert np.array_equal(CR.apply64([ONE] * 3, x), x) and np.array_equal(CR.adjoint64([ONE] * 3, x), x)
    assert np.array_equal(CR.w64(CR.TAPS, 0.0), (CR.TAPS == 0).astype(np.float64))
    assert np.array_equal(CR.w32(CR.TAPS, np.float32(0)), (CR.TAPS == 0).astype(np.float32))
    assert CR.rq_of(1.0) == ONE and CR.clamp_rq(1) == 1 << 31 and CR.clamp_rq(1 << 40) == 1 << 33


def test_draw_against_hand_computed_words():
    # Philox4x32-10 of the zero counter under the zero key (Random123's known answer), then the draw's own arithmetic by hand
    assert PR.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    seed, step, clip, stream, D = 5 + (9 << 32), 3, 17, 1, CR.drift_q32(20000.0)
    assert D == 85899346                                                   # round(0.02 * 2^32)
    c = PR.philox4x32_10((step, clip, stream, 2), (5, 9))
    rq, snr = CR.draw_one(seed, step, clip, stream, D, 10.0, 30.0)
    assert rq == ONE + ((c[0] - 2 ** 31) * D // 2 ** 31)                   # floor division = the arithmetic shift
    assert snr == np.float32(10.0 + 20.0 * ((c[1] >> 8) / 2.0 ** 24))
    lo_hi = [CR.draw(seed, s, 0, 64, 0, D, 10.0, 30.0) for s in range(4)]
    allrq = [q for rqs, _ in lo_hi for q in rqs]
    assert all(ONE - D <= q <= ONE + D for q in allrq) and len(set(allrq)) == len(allrq)
    assert min(allrq) < ONE - D // 2 and max(allrq) > ONE + D // 2         # both halves of 1 +- eps are reached
    assert all(10.0 <= s <= 30.0 for _, ss in lo_hi for s in ss)
    assert CR.draw(seed, 0, 0, 4, 0, 0)[0] == [ONE] * 4                    # drift off: exactly one
    # the extreme words
    assert ONE + (((0 - 2 ** 31) * D) >> 31) == ONE - D and ONE + (((2 ** 32 - 1 - 2 ** 31) * D) >> 31) == ONE + D - 1


def test_philox_streams_are_disjoint():
    """(counter, key) of the four uses under one seed: the draws differ in counter word 3 (0, 1, 2, constants of the code), the
    noise in the key — for EVERY seed, step, clip, stream and sample, since k1 ^ NOISE_KEY != k1."""
    assert CR.NOISE_KEY != 0 and len({CR.TAG_PLACE, CR.TAG_ROOM, CR.TAG_CHAN}) == 3
    for seed in (0, 5, (1 << 64) - 1, CR.NOISE_KEY << 32):
        assert CR.key_of(seed, True) != CR.key_of(seed) and CR.key_of(seed, True)[0] == CR.key_of(seed)[0]
        seen = {}
        for step in range(3):
            for clip in range(3):
                for stream in range(3):
                    for tag, name in ((CR.TAG_PLACE, "place"), (CR.TAG_ROOM, "room")):
                        seen.setdefault(((step, clip, stream, tag), CR.key_of(seed)), name)
                    assert CR.draw_counter(step, clip, stream)[3] == CR.TAG_CHAN
                    seen.setdefault((CR.draw_counter(step, clip, stream), CR.key_of(seed)), "chan")
                    for group in range(4):          # a noise counter may equal a draw's counter: word 2 = group, word 3 = stream
                        seen.setdefault((CR.noise_counter(step, clip, group, stream), CR.key_of(seed, True)), "noise")
        names = list(seen.values())
        assert names.count("place") == names.count("room") == names.count("chan") == 27 and names.count("noise") == 108
    # the placement and room references really use those tags
    import rir_ref as RR
    assert PR.draw_raw(5, 1, 2, 0) == PR.philox4x32_10((1, 2, 0, CR.TAG_PLACE), (5, 0))
    assert RR.draw_room(5, 1, 2, 0, 1 << 20) == (PR.philox4x32_10((1, 2, 0, CR.TAG_ROOM), (5, 0))[0] << 20) >> 32


def test_float32_weights_within_three_units_of_float64():
    rng = np.random.default_rng(12345)
    f = rng.random(20000, dtype=np.float32)
    f[:4] = [0.0, np.float32(2.0 ** -24), np.float32(1.0 - 2.0 ** -24), 0.5]
    w32 = CR.w32(CR.TAPS[None, :], f[:, None]).astype(np.float64)
    w64 = CR.w64(CR.TAPS[None, :], f[:, None].astype(np.float64))
    worst = float(np.abs(w32 - w64).max() / 2.0 ** -24)
    print(f"float32 weights: worst |w32 - w64| = {worst:.3f} units of 2^-24")
    assert worst <= 3.0
    # partition of unity up to the window's ripple, as DESIGN.md 6k states it
    assert float(np.abs(w64.sum(axis=1) - 1.0).max()) < 5e-4


def test_reference_noise_is_standard_normal():
    n = 1 << 16
    z = CR.noise64(5, 0, 0, 0, n)                                           # seed 5: pinned
    assert abs(z.mean()) < 5.0 / np.sqrt(n) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert np.isfinite(z).all() and 3.5 < np.abs(z).max() < 6.0
    assert not np.array_equal(z[:64], CR.noise64(5, 1, 0, 0, 64)) and not np.array_equal(z[:64], CR.noise64(5, 0, 1, 0, 64))
    assert not np.array_equal(z[:64], CR.noise64(5, 0, 0, 1, 64))
    assert np.array_equal(z[:61], CR.noise64(5, 0, 0, 0, 61))               # a sample does not depend on L
    x = np.ones((2, 100)) * 0.5
    assert np.allclose(CR.sigma64(x, [20.0, 0.0]), [0.05, 0.5])


# ---- flags, modes, refusals ----------------------------------------------------------------------------------------------
def _args(**kw):
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_parser_defaults_and_flags():
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args([])
    assert a.drift_ppm == 0.0 and a.noise_snr_db is None
    a = parser.create_arg_parser().parse_args(["--drift_ppm", "500", "--noise_snr_db", "10", "30"])
    assert a.drift_ppm == 500.0 and list(a.noise_snr_db) == [10.0, 30.0]
    for bad in (["--drift_ppm", "-1"], ["--drift_ppm", "100001"], ["--noise_snr_db", "10"], ["--noise_snr_db", "-21", "0"],
                ["--noise_snr_db", "0", "101"]):
        with pytest.raises(SystemExit):
            parser.create_arg_parser().parse_args(bad)


def test_on_off_rule_suffix_and_results():
    from paa_amd.training_utils import channel, place, rir
    from paa_amd.training_utils.modes import Modes
    assert not channel.chan_on(types.SimpleNamespace()) and not channel.chan_on(_args())
    m = Modes.of(types.SimpleNamespace())
    assert (m.chan_on, m.drift_on, m.noise_on, m.drift_ppm, m.noise_snr) == (False, False, False, 0.0, None)
    d, n, both = _args(drift_ppm=500.0), _args(noise_snr_db=[10.0, 30.0]), _args(drift_ppm=2.5, noise_snr_db=[20.0, 20.0])
    assert Modes.of(d).drift_on and not Modes.of(d).noise_on and Modes.of(d).chan_on
    assert Modes.of(n).noise_on and not Modes.of(n).drift_on and Modes.of(n).chan_on
    assert not place.placement_on(both) and not rir.rir_on(both)                # the other modes keep their meaning
    assert channel.suffix(_args()) == "" and channel.results_extra(_args()) == {}
    assert channel.suffix(d) == "_drift500" and channel.suffix(n) == "_noise10-30" and channel.suffix(both) == "_drift2.5_noise20-20"
    assert channel.results_extra(d) == {"drift_ppm": 500.0} and channel.results_extra(n) == {"noise_snr_db": [10.0, 30.0]}
    assert channel.results_extra(both) == {"drift_ppm": 2.5, "noise_snr_db": [20.0, 20.0]}
    assert channel.drift_q32(20000.0) == CR.drift_q32(20000.0) and channel.rq_of(0.9) == CR.rq_of(0.9)
    assert channel.rq_of(0.1) == 1 << 31 and channel.rq_of(5.0) == 1 << 33


def test_refusals_without_gpu(monkeypatch):
    from paa_amd import attack_clips, run_attack
    from paa_amd.training_utils import channel, evaluation, modes, train
    from paa_amd.training_utils.pgd import PgdStepper, lengths_refusal
    model = types.SimpleNamespace(device=torch.device("cpu"), max_batch=2, length=16000, lengths_on=False)
    on = (dict(drift_ppm=500.0), dict(noise_snr_db=[10.0, 30.0]))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setenv("WORLD_SIZE", "1")

    def entries(a):
        """Every entry point up to its refusals."""
        yield lambda: channel.check(a)
        yield lambda: PgdStepper(model, a, 16000)
        yield lambda: evaluation._PlacedEval(a, model, torch.zeros(1, 16000))
        yield lambda: run_attack.main(a)

    # the masking norm / loss pair delta's frames with the clean clip's: drift unpairs them
    for kw in on:
        for a in (_args(norm_type="masking", **kw), _args(norm_type="linf+masking", **kw), _args(norm_type="linf", masking_loss_alpha=0.5, **kw)):
            with pytest.raises(NotImplementedError, match=r"playback channel \(drift_ppm / noise_snr_db\) is not implemented with the masking"):
                channel.check_flags(a)
            for f in entries(a):
                with pytest.raises(NotImplementedError, match="playback channel"):
                    f()
    channel.check(_args(norm_type="masking"))                                   # the mode off: nothing to refuse
    channel.check(_args(norm_type="masking"), eager_adam=True)
    # the eager-Adam route
    for kw in on:
        with pytest.raises(NotImplementedError, match=r"playback channel \(drift_ppm / noise_snr_db\) needs the device step"):
            channel.check(_args(norm_type="linf", **kw), eager_adam=True)
        p = torch.nn.Parameter(torch.zeros(1, 16000))
        opt = torch.optim.Adam([p], lr=0.1, weight_decay=0.1)                   # an optimizer the device step does not cover
        with pytest.raises(NotImplementedError, match="playback channel"):
            train.train_epoch(_args(norm_type="linf", optimizer_type="adam", **kw), [], p, model, 0, None, None, None, None, opt)
    # the ranges, through a hand-built namespace; judged with the mode off too (a negative drift is no "off")
    for kw, name in ((dict(drift_ppm=-1.0), "drift_ppm"), (dict(drift_ppm=100001.0), "drift_ppm"), (dict(drift_ppm=float("nan")), "drift_ppm"),
                     (dict(noise_snr_db=[30.0, 10.0]), "noise_snr_db"), (dict(noise_snr_db=[-21.0, 10.0]), "noise_snr_db"),
                     (dict(noise_snr_db=[10.0, 101.0]), "noise_snr_db"), (dict(noise_snr_db=[10.0]), "noise_snr_db")):
        a = _args(norm_type="linf", **kw)
        with pytest.raises(ValueError, match=name + " must be"):
            channel.check_flags(a)
        for f in entries(a):
            with pytest.raises(ValueError, match=name):
                f()
        with pytest.raises(ValueError, match=name):
            channel.suffix(a)
    # true clip lengths
    for kw in on:
        a = _args(norm_type="linf", clip_lengths="true", **kw)
        with pytest.raises(ValueError, match="--clip_lengths true does not support --drift_ppm / --noise_snr_db"):
            modes.check(modes.Modes.of(a), modes.LENGTHS)
        with pytest.raises(ValueError, match="--drift_ppm / --noise_snr_db"):
            run_attack.main(a)
        with pytest.raises(ValueError, match="--drift_ppm / --noise_snr_db"):
            evaluation.evaluate(a, [], 0, model, None, None)
        assert "--drift_ppm" in lengths_refusal(_args(norm_type="linf", **kw))
    assert lengths_refusal(_args(norm_type="linf")) is None
    # per-clip perturbations have no channel yet
    for flags in (["--drift_ppm", "500"], ["--noise_snr_db", "10", "30"]):
        with pytest.raises(NotImplementedError, match=r"--drift_ppm / --noise_snr_db apply to the universal perturbation .*per-clip"):
            attack_clips.main(attack_clips.create_arg_parser().parse_args(flags))
    with pytest.raises(NotImplementedError, match="per-clip"):
        channel.refuse_for_clips(_args(drift_ppm=1.0))
    channel.refuse_for_clips(_args())
    # the rules sit where their neighbours sit
    assert modes.CHANNEL == ("chan_range", "chan_masking", "chan_eager") and "len_chan" in modes.LENGTHS
    for k in ("chan_range", "chan_masking", "chan_eager", "chan_clips", "len_chan"):
        assert k in modes.RULES
    same = lambda a, b, x, y: modes.RULES[a].msg.replace(x, "@") == modes.RULES[b].msg.replace(y, "@")
    assert same("chan_masking", "rir_masking", "the playback channel (drift_ppm / noise_snr_db) is", "room responses (rir_bank) are")
    assert same("chan_eager", "rir_eager", "the playback channel (drift_ppm / noise_snr_db) needs", "room responses (rir_bank) need")
    assert same("len_chan", "len_rir", "--drift_ppm / --noise_snr_db", "--rir_bank")
    assert modes.RULES["chan_clips"].msg.replace("--drift_ppm / --noise_snr_db apply", "@").replace("playback channel", "#") == \
        modes.RULES["rir_clips"].msg.replace("--rir_bank applies", "@").replace("room responses", "#")


def test_channel_object_checks_its_arguments_on_the_host():
    from paa_amd.training_utils import channel
    with pytest.raises(ValueError, match="drift_ppm"):
        channel.Channel(torch.device("cpu"), 2, 100, 0, 0, drift_ppm=-3.0)
    with pytest.raises(ValueError, match="noise_snr_db"):
        channel.Channel(torch.device("cpu"), 2, 100, 0, 0, noise_snr=(5.0, 1.0))
    ch = channel.Channel(torch.device("cpu"), 2, 100, 7, 1, drift_ppm=1000.0, noise_snr=(10.0, 20.0), clip_base=4)
    assert ch.drift_on and ch.noise_on and ch.D == CR.drift_q32(1000.0) and ch.rq.tolist() == [ONE, ONE]
    assert ch.rows.shape == (2, 100) and ch.grad_rows.shape == (2, 100) and not ch.explicit
    ch.set_channel([0.9, ONE + 5], [12.0, 13.0])
    assert ch.explicit and ch.rq.tolist() == [CR.rq_of(0.9), ONE + 5] and ch.snr_db.tolist() == [12.0, 13.0]
    ch.set_channel(None)
    assert not ch.explicit
    for bad in ([1.0, 1.0, 1.0], [0.4, 1.0], [1.0, 2.5]):
        with pytest.raises(ValueError):
            ch.set_channel(bad)
    with pytest.raises(ValueError):
        ch.set_channel([1.0, 1.0], [10.0])
    ch.set_step(9)
    assert int(ch.counter) == 9 and int(ch.noise_counter) == 9
    off = channel.Channel(torch.device("cpu"), 2, 100, 7, 1, noise_snr=(10.0, 20.0))
    assert off.rows is None and not off.drift_on
    with pytest.raises(RuntimeError, match="drift off"):
        off.apply(torch.zeros(2, 100), 2)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from paa_amd import _lib
    return _lib


def test_new_entries_declared_exported_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "paa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(paa_[a-z0-9_]+)\s*\(", hdr))
    L = lib.lib()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in lib.exported_symbols(), name
        assert hasattr(L, name), name
    assert L.paa_version() in (350, 351)                                       # pure additions: no new number
    from paa_amd import build_ext
    assert "chan_kernels.hip" in build_ext.SOURCES


def test_new_entries_refuse_before_any_launch(lib):
    L = lib.lib()
    d, e = C.c_void_p(1 << 20), C.c_void_p(1 << 24)        # never dereferenced: the arguments are refused first
    ARG = lib.PAA_ERR_ARG
    for k in range(3):
        a = [d, d, e]
        a[k] = None
        for adj in (0, 1):
            assert L.paa_drift_apply(a[0], a[1], a[2], 2, 100, adj, None) == ARG
    for B_, L_ in ((0, 100), (2, 0), (-1, 100)):
        for adj in (0, 1):
            assert L.paa_drift_apply(d, d, e, B_, L_, adj, None) == ARG
    assert b"paa_drift_apply" in L.paa_last_error()
    for off in (0, 4, 2 * 100 * 4 - 4, -(2 * 100 * 4 - 4)):
        assert L.paa_drift_apply(d, e, C.c_void_p((1 << 24) + off), 2, 100, 0, None) == ARG
        assert b"overlap" in L.paa_last_error()
    assert L.paa_chan_draw(5, None, 0, 0, 2, 10, 0.0, 1.0, d, d, None) == ARG
    assert L.paa_chan_draw(5, d, 0, 0, 2, 10, 0.0, 1.0, None, d, None) == ARG
    assert L.paa_chan_draw(5, d, 0, 0, 2, 10, 0.0, 1.0, d, None, None) == ARG
    assert L.paa_chan_draw(5, d, 0, 0, 0, 10, 0.0, 1.0, d, d, None) == ARG
    assert L.paa_chan_draw(5, d, 0, 0, 2, (1 << 31) + 1, 0.0, 1.0, d, d, None) == ARG
    assert L.paa_chan_draw(5, d, 0, 0, 2, 10, 1.0, 0.0, d, d, None) == ARG
    assert b"paa_chan_draw" in L.paa_last_error()
    for k in range(5):
        a = [d, d, d, d, e]
        a[k] = None
        assert L.paa_noise_add(5, a[0], 0, 0, a[1], a[2], a[3], a[4], 2, 100, None) == ARG
    assert L.paa_noise_add(5, d, 0, 0, d, d, d, e, 0, 100, None) == ARG and L.paa_noise_add(5, d, 0, 0, d, d, d, e, 2, 0, None) == ARG
    assert b"paa_noise_add" in L.paa_last_error()
