"""No-GPU checks of the placement layer: the Python Philox of tests/place_ref.py against known answers, place / reduce against
torch float64 autograd, the parser's new flags, the on / off rule, every refusal that needs no GPU and the C-ABI entries."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import place_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_place_draw", "paa_place_rows", "paa_place_reduce")


def _hex(words):
    return " ".join(f"{w:08x}" for w in words)


def test_philox_known_answers():
    assert _hex(PR.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(PR.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(PR.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


@pytest.mark.parametrize("Lp,want", [(1000, [765, 932, 734, 347]), (16000, [12255, 14915, 11758, 5555])])
def test_shift_table(Lp, want):
    got = [PR.draw_shift(5, step, clip, 0, Lp) for step, clip in ((0, 0), (0, 1), (0, 2), (1, 0))]
    assert got == want
    assert PR.draw_shift(5, 0, 0, 0, Lp, shift_on=False) == 0
    assert PR.draw_shift(5, 0, 0, 1, Lp) != got[0]          # the evaluation stream draws its own


def test_gain_draw():
    assert PR.draw_gain64(5, 0, 0, 0, 0.0) == 1.0
    g = [PR.draw_gain_db(5, s, c, 0, 6.0) for s in range(8) for c in range(8)]
    assert all(-6.0 <= float(x) < 6.0 for x in g) and len(set(float(x) for x in g)) == 64


@pytest.mark.parametrize("B,L,Lp", [(3, 50, 50), (3, 50, 16), (2, 87, 40), (3, 50, 70), (2, 60, 1), (2, 60, 3)])
def test_place_and_adjoint_vs_autograd(B, L, Lp):
    rng = np.random.default_rng(B * 1000 + L + Lp)
    p = rng.standard_normal(Lp)
    shift = [0, Lp - 1, Lp + 5][:B] if B == 3 else [1 % Lp, -1]
    gain = [0.5, 1.0, 1.7][:B]
    G = rng.standard_normal((B, L))
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    idx = (torch.arange(L)[None, :] + torch.tensor(np.mod(shift, Lp))[:, None]) % Lp
    rows = pt[idx] * torch.tensor(gain, dtype=torch.float64)[:, None]
    (rows * torch.tensor(G)).sum().backward()
    got = PR.place(p, L, shift, gain, dtype=np.float64)
    assert np.array_equal(got, rows.detach().numpy())
    grad, mag, cnt = PR.reduce64(G, shift, gain, Lp)
    np.testing.assert_allclose(grad, pt.grad.numpy(), rtol=1e-13, atol=1e-14)
    assert int(cnt.sum()) == B * L
    if Lp > L:
        untouched = cnt == 0
        assert untouched.any() and np.all(grad[untouched] == 0) and np.all(pt.grad.numpy()[untouched] == 0)
    # <rows(p), G> = <p, reduce(G)>
    assert abs(float((got * G).sum()) - float((p * grad).sum())) <= 1e-12 * float(np.abs(got * G).sum())
    # Lp = L, shift 0, no gain: the broadcast
    if Lp == L:
        assert np.array_equal(PR.place(p.astype(np.float32), L, [0] * B), np.broadcast_to(p.astype(np.float32), (B, L)))


def test_parser_defaults_and_flags():
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args([])
    assert a.perturbation_seconds is None and a.place_shift == "none" and a.place_gain_db == 0.0
    a = parser.create_arg_parser().parse_args(["--perturbation_seconds", "1.5", "--place_shift", "random", "--place_gain_db", "6"])
    assert a.perturbation_seconds == 1.5 and a.place_shift == "random" and a.place_gain_db == 6.0
    for bad in (["--place_shift", "always"], ["--place_gain_db", "-1"], ["--place_gain_db", "20.5"]):
        with pytest.raises(SystemExit):
            parser.create_arg_parser().parse_args(bad)


def _args(**kw):
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_on_off_rule():
    from paa_amd.training_utils import place
    assert not place.placement_on(types.SimpleNamespace())                    # callers that never heard of the flags
    assert not place.placement_on(_args())
    assert place.placement_on(_args(perturbation_seconds=10.0))               # even at the clip length
    assert place.placement_on(_args(place_shift="random"))
    assert place.placement_on(_args(place_gain_db=3.0))
    assert place.perturbation_length(_args(), 160000) == 160000
    assert place.perturbation_length(_args(perturbation_seconds=1.0), 160000) == 16000
    assert place.perturbation_length(_args(perturbation_seconds=0.256), 160000) == 4096
    with pytest.raises(ValueError):
        place.perturbation_length(_args(perturbation_seconds=0.0), 160000)
    # the run directory and results.json change only with placement on
    assert place.suffix(_args()) == "" and place.results_extra(_args(), 160000) == {}
    on = _args(perturbation_seconds=1.0, place_shift="random", place_gain_db=6.0)
    assert place.suffix(on) == "_place16000sg6"
    assert place.results_extra(on, 16000) == {"perturbation_length": 16000, "place_shift": "random", "place_gain_db": 6.0}


def test_refusals_without_gpu():
    from paa_amd import attack_clips
    from paa_amd.training_utils import place
    from paa_amd.training_utils.pgd import PgdStepper
    model = types.SimpleNamespace(device=torch.device("cpu"), max_batch=2, length=16000)
    # the masking norm / loss pair delta's frames with the clean clip's
    for a in (_args(norm_type="masking", place_shift="random"), _args(norm_type="linf+masking", place_gain_db=3.0),
              _args(norm_type="linf", masking_loss_alpha=0.5, perturbation_seconds=1.0)):
        with pytest.raises(NotImplementedError, match="masking"):
            place.check(a, 16000, 16000)
        with pytest.raises(NotImplementedError, match="masking"):
            PgdStepper(model, a, 16000)                                       # raised before anything touches a device
    with pytest.raises(NotImplementedError, match="masking"):
        place.check_flags(_args(norm_type="masking", place_shift="random"))   # the runner's check before any collective
    place.check_flags(_args(norm_type="snr", perturbation_seconds=0.5))       # what depends on the lengths is check()'s
    place.check_flags(_args(norm_type="masking"))
    # snr / tv with a perturbation of another length
    for n in ("snr", "tv", "linf+tv"):
        a = _args(norm_type=n, perturbation_seconds=0.5)
        with pytest.raises(NotImplementedError, match="snr / tv"):
            PgdStepper(model, a, 16000)
        place.check(_args(norm_type=n, place_shift="random"), 16000, 16000)   # Lp = L: fine
    # the eager-Adam route
    with pytest.raises(NotImplementedError, match="device step"):
        place.check(_args(norm_type="linf", place_shift="random"), 16000, 16000, eager_adam=True)
    place.check(_args(norm_type="masking"), 16000, 16000, eager_adam=True)    # placement off: nothing to refuse
    # values outside the flags' ranges reaching the stepper through a hand-built namespace
    with pytest.raises(ValueError, match="place_gain_db"):
        place.check(_args(norm_type="linf", place_gain_db=21.0), 16000, 16000)
    with pytest.raises(ValueError, match="place_shift"):
        place.check(_args(norm_type="linf", place_shift="always", place_gain_db=1.0), 16000, 16000)
    # a p_length of its own needs placement on
    with pytest.raises(ValueError, match="p_length"):
        PgdStepper(model, _args(norm_type="linf"), 16000, p_length=4096)
    # per-clip rows have no placement
    for extra in (["--perturbation_seconds", "1"], ["--place_shift", "random"], ["--place_gain_db", "3"]):
        with pytest.raises(NotImplementedError, match="per-clip"):
            attack_clips.main(attack_clips.create_arg_parser().parse_args(extra))


def test_hop_warning_logged_once(caplog):
    from paa_amd.training_utils import place
    a = _args(norm_type="max_phon", perturbation_seconds=1000 / 16000)
    with caplog.at_level("WARNING", logger=place.logger.name):
        place.check(a, 16000, 1000)
        place.check(a, 16000, 1000)
        place.check(_args(norm_type="linf", perturbation_seconds=1000 / 16000), 16000, 1000)     # no frequency-domain norm
    assert len([r for r in caplog.records if "hop_length" in r.getMessage()]) == 1


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
    assert L.paa_version() in lib.ABI_VERSIONS and lib.ABI_VERSIONS == (350, 351)


def test_new_entries_refuse_before_any_launch(lib):
    L = lib.lib()
    d = C.c_void_p(16)        # never dereferenced: the arguments are refused first
    ARG = lib.PAA_ERR_ARG
    assert L.paa_place_draw(5, None, 0, 0, 2, 100, 1, 0.0, d, d, None) == ARG
    assert L.paa_place_draw(5, d, 0, 0, 2, 100, 1, 0.0, None, d, None) == ARG
    assert L.paa_place_draw(5, d, 0, 0, 2, 100, 1, 0.0, d, None, None) == ARG
    assert L.paa_place_draw(5, d, 0, 0, 0, 100, 1, 0.0, d, d, None) == ARG
    assert L.paa_place_draw(5, d, 0, 0, 2, 0, 1, 0.0, d, d, None) == ARG
    for g in (-0.5, 20.5, float("nan")):
        assert L.paa_place_draw(5, d, 0, 0, 2, 100, 1, g, d, d, None) == ARG
    assert b"gain_db" in L.paa_last_error()
    assert L.paa_place_rows(None, 100, d, None, d, 2, 100, None) == ARG
    assert L.paa_place_rows(d, 100, None, None, d, 2, 100, None) == ARG
    assert L.paa_place_rows(d, 100, d, None, None, 2, 100, None) == ARG
    for B_, L_, Lp_ in ((0, 100, 100), (2, 0, 100), (2, 100, 0), (-1, 100, 100)):
        assert L.paa_place_rows(d, Lp_, d, None, d, B_, L_, None) == ARG
        assert L.paa_place_reduce(d, d, d, d, B_, L_, Lp_, None) == ARG
    for k in range(4):
        a = [d, d, d, d]
        a[k] = None
        assert L.paa_place_reduce(*a, 2, 100, 100, None) == ARG
