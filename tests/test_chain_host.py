"""No-GPU checks of training_utils/chain.py (DESIGN.md "The playback chain"): the sites of a ``PlaybackChain`` built on the CPU
device — which counters a capture hands back, which a resume sets, how ``clip_base`` reaches every site — and ``chain.check`` /
``check_flags`` / ``suffix`` / ``results_extra`` against the three links' own calls in the chain's order."""
import copy
import itertools
import json
import types

import pytest
import torch

import test_modes_host as TM

L, NB = 400, 3
ON = {"place": dict(place_shift="random"), "rir": dict(rir_bank="synthetic", rir_count=2, rir_taps=16),
      "drift": dict(drift_ppm=500.0), "noise": dict(noise_snr_db=[10.0, 30.0])}


def _args(**kw):
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args(["--norm_type", "linf"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _chain(modes, rank=0):
    from paa_amd.training_utils import chain, place
    model = types.SimpleNamespace(device=torch.device("cpu"), max_batch=NB, length=L)
    return chain.PlaybackChain(_args(**{k: v for m in modes for k, v in ON[m].items()}), model, L, place.STREAM_TRAIN, True, rank)


COMBOS = [c for n in range(1, 5) for c in itertools.combinations(ON, n)]


@pytest.mark.parametrize("modes", COMBOS, ids="+".join)
def test_counters_set_step_and_clip_base(modes):
    ch = _chain(modes, rank=2)
    chan_on = "drift" in modes or "noise" in modes
    assert (ch.reverb is not None) == ("rir" in modes) and (ch.chan is not None) == chan_on
    assert ch.placer.explicit == ("place" not in modes)          # placement off: pinned at shift 0, gain 1, nothing drawn
    # counters(): the sites whose mode is on, in the order place, rooms, channel draw, channel noise
    want = ([ch.placer.counter] if "place" in modes else []) + ([ch.reverb.counter] if "rir" in modes else []) \
        + ([ch.chan.counter, ch.chan.noise_counter] if chan_on else [])
    got = ch.counters()
    assert len(got) == len(want) and all(g is w for g, w in zip(got, want))
    # set_step: those counters and no other — with placement off the placer's stays where it is
    ch.placer.counter.fill_(7)
    ch.set_step(40)
    assert [int(c) for c in ch.counters()] == [40] * len(want)
    assert int(ch.placer.counter) == (40 if "place" in modes else 7)
    # clip_base: rank * max_batch at every site, and an assignment reaches every site
    sites = [s for s in (ch.placer, ch.reverb, ch.chan) if s is not None]
    assert ch.clip_base == 2 * NB and all(s.clip_base == 2 * NB for s in sites)
    ch.clip_base = 11
    assert ch.clip_base == 11 and all(s.clip_base == 11 for s in sites)
    assert all(s._base(None) == 11 and s._base(5) == 5 for s in sites)


def test_site_checks_and_unpin():
    ch = _chain(("rir", "drift"))
    for s in (ch.placer, ch.reverb, ch.chan):
        for B in (0, NB + 1):
            with pytest.raises(ValueError, match=rf"batch {B} outside \[1, {NB}\]"):
                s._fits(B)
        for bad in (None, torch.zeros(2, L, dtype=torch.float64), torch.zeros(2, 2 * L)[:, ::2], torch.zeros(1, L)):
            with pytest.raises(ValueError, match=rf"rows must be contiguous float32 with at least 2 x {L} elements"):
                s._check_rows(bad, 2)
        s._check_rows(torch.zeros(NB, L), 2)
    with pytest.raises(ValueError, match=rf"clean must be contiguous float32 with at least 1 x {L} elements"):
        ch.chan._check_rows(None, 1, "clean")
    ch.reverb.set_rooms([1, 0])
    ch.chan.set_channel([1.0, 0.99])
    assert ch.placer.explicit and ch.reverb.explicit and ch.chan.explicit
    ch.placer.set_placement(None), ch.reverb.set_rooms(None), ch.chan.set_channel(None)
    assert not (ch.placer.explicit or ch.reverb.explicit or ch.chan.explicit)
    assert type(ch.placer)(torch.device("cpu"), 1, 4, 4, (1 << 64) + 5, 0, False, 0.0).seed == 5          # masked to 64 bits


def _outcome(f):
    """What ``f`` returns, or what it raises."""
    try:
        return repr(f())
    except Exception as e:      # noqa: BLE001
        return f"{type(e).__name__}: {e}"


# the channel's flags are no axis of the recorded grid: every row is crossed with these
CHANNELS = [{}, {"drift_ppm": 500.0}, {"noise_snr_db": [10.0, 30.0]}, {"drift_ppm": -1.0}]


def test_check_is_the_three_links_in_order():
    """On the rows of tests/golden/mode_refusals.json with placement or room responses on (crossed with the channel's flags),
    ``chain.check`` raises what ``place.check; rir.check; channel.check`` raise first, and so do the flag-only and naming helpers.
    Where the channel's flags are the row's own, that refusal is also the one the fixture recorded for ``train_epoch``, which walks
    alpha_eager, then the chain, then the lengths (off in these rows)."""
    from paa_amd import attack_clips
    from paa_amd.training_utils import chain, channel, place, rir
    from paa_amd.training_utils.modes import RULES, Modes
    with open(TM.FIXTURE) as f:
        fx = json.load(f)
    assert fx["grid"] == TM.GRID and fx["extras"] == TM.EXTRAS and fx["L"] == TM.L and fx["entries"] == TM.ENTRIES
    recorded = [fx["messages"][row[TM.ENTRIES.index("train_epoch")]] for row in fx["cases"]]
    alpha_eager = f"{RULES['alpha_eager'].exc.__name__}: {RULES['alpha_eager'].msg}"
    base = attack_clips.create_arg_parser().parse_args([])
    base.rir_count, base.rir_taps, base.optimizer_type = 2, 16, "adam"
    seen, raised, matched = 0, set(), 0
    for pt, rec in zip(TM.points(), recorded):
        if pt["world"] != 1 or pt["clip_lengths"] != "padded":          # neither is an argument of the chain's checks
            continue
        for extra in CHANNELS:
            args = copy.copy(base)
            for k, v in {**pt, **extra}.items():
                if k not in ("world", "eager_adam"):
                    setattr(args, k, v)
            m = Modes.of(args)
            if not (m.place_on or m.rir_on or m.chan_on or extra):
                continue
            eager = pt["eager_adam"]
            Lp = place.perturbation_length(args, TM.L)

            def three():
                place.check(args, TM.L, Lp, eager)
                rir.check(args, eager)
                channel.check(args, eager)

            def three_flags():
                place.check_flags(args)
                rir.check_flags(args)
                channel.check_flags(args)

            want = _outcome(three)
            if not extra and rec != alpha_eager:
                assert want == ("None" if rec == "none" else rec), (pt, want, rec)
                matched += 1
            assert _outcome(lambda: chain.check(args, TM.L, Lp, eager)) == want, (pt, extra)
            assert _outcome(lambda: chain.check_flags(args)) == _outcome(three_flags), (pt, extra)
            assert _outcome(lambda: chain.suffix(args)) == \
                _outcome(lambda: place.suffix(args) + rir.suffix(args) + channel.suffix(args)), (pt, extra)
            assert _outcome(lambda: sorted(chain.results_extra(args, Lp).items())) == \
                _outcome(lambda: sorted({**place.results_extra(args, Lp), **rir.results_extra(args),
                                         **channel.results_extra(args)}.items())), (pt, extra)
            seen += 1
            raised.add(want)
    # no vacuous walk: refusals of all three links win somewhere, and so does no refusal at all
    assert seen > 500 and matched > 100 and "None" in raised
    for part in ("placement (", "room responses (rir_bank)", "the playback channel (", "drift_ppm must be", "rir_count must be"):
        assert any(part in r for r in raised), part
