"""CPU: the float64 statement of the alignment-margin loss (tests/align_ref.py) against brute force and torch's
float64 autograd, the two mode rules, the flags, and the three C entries against the header."""
import itertools
import os
import re

import numpy as np
import pytest

import align_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 0
NEW_ENTRIES = ("paa_align_margin", "paa_align_margin_work_floats", "paa_model_set_loss")


def _collapse(path):
    out, prev = [], None
    for c in path:
        if c != prev and c != BLANK:
            out.append(int(c))
        prev = c
    return out


# (T, labels): S = 0..3 at V = 4, with a repeated label (which needs the blank between), at and above the minimum frame count
BRUTE = [(1, []), (4, []), (3, [2]), (5, [1, 2]), (3, [3, 3]), (6, [3, 3]), (7, [1, 1, 2]), (7, [2, 3, 1]), (5, [2, 2, 2]), (6, [1, 3, 3])]


@pytest.mark.parametrize("T,labels", BRUTE, ids=[f"T{t}-{'-'.join(map(str, l)) or 'empty'}" for t, l in BRUTE])
def test_reference_path_is_the_unique_brute_force_maximiser(T, labels):
    V = 4
    rng = np.random.default_rng(100 * T + len(labels))
    z = rng.standard_normal((T, V)).astype(np.float32)
    row = np.asarray(labels + [-1], dtype=np.int32)
    scored = []
    for path in itertools.product(range(V), repeat=T):
        if _collapse(path) == labels:
            scored.append((float(np.sum(z[np.arange(T), list(path)].astype(np.float64))), path))
    assert scored, "the case must be feasible"
    scored.sort(reverse=True)
    if len(scored) > 1:
        assert scored[0][0] - scored[1][0] > 1e-9, "continuous logits: the maximiser is unique"
    pi, best = AR.forced_alignment(z, row, BLANK, with_value=True)
    assert tuple(int(c) for c in pi) == scored[0][1]
    assert abs(best - scored[0][0]) < 1e-12


def test_infeasible_rows_have_no_path():
    z = np.zeros((2, 4), dtype=np.float32)
    assert AR.forced_alignment(z, np.asarray([1, 1]), BLANK) is None           # a a needs 3 frames
    assert AR.forced_alignment(z, np.asarray([1, 2, 3]), BLANK) is None
    assert AR.forced_alignment(z, np.asarray([1, 2]), BLANK) is not None
    out = AR.align_margin(np.zeros((2, 2, 4), np.float32), np.asarray([[1, 1], [1, 2]]), BLANK, 1.0)
    assert np.isinf(out["loss"][0]) and np.isnan(out["dlogits"][0]).all() and np.isfinite(out["loss"][1])
    assert not np.isnan(out["dlogits"][1]).any() and (out["align"][0] == BLANK).all()


def test_tie_rule_hand_example():
    """All-zero logits, T = 5, labels (a, a): stay over s-1 over s-2, state 2S over 2S-1 -> a 0 a 0 0."""
    pi = AR.forced_alignment(np.zeros((5, 4), dtype=np.float32), np.asarray([1, 1]), BLANK)
    assert pi.tolist() == [1, 0, 1, 0, 0]
    assert AR.forced_alignment(np.zeros((3, 4), dtype=np.float32), np.asarray([-1, -1]), BLANK).tolist() == [0, 0, 0]
    assert AR.extended([-1, 3, -1, 3, 2, -1], BLANK).tolist() == [0, 3, 0, 3, 0, 2, 0]


@pytest.mark.parametrize("kappa", [0.0, 1.0, 2.5])
def test_hinge_value_and_cotangent_against_float64_autograd(kappa):
    import torch
    rng = np.random.default_rng(41)
    B, T, V = 3, 30, 9
    logits = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    labels = np.asarray([[1, 2, 2, 5, -1], [3, -1, -1, -1, -1], [8, 7, 7, 7, 1]], dtype=np.int32)
    frames = [30, 12, 25]
    out = AR.align_margin(logits, labels, BLANK, kappa, 1.0, frames)
    for b in range(B):
        tb = frames[b]
        pi = torch.from_numpy(out["align"][b, :tb].astype(np.int64))
        z = torch.tensor(logits[b, :tb], dtype=torch.float64, requires_grad=True)
        rest = z.masked_fill(torch.nn.functional.one_hot(pi, V).bool(), -float("inf"))
        top2 = rest.topk(2, dim=1).values
        m = np.float64(np.float32(kappa)) + top2[:, 0] - z.gather(1, pi[:, None])[:, 0]
        # the draw keeps every frame off the hinge's edge and every runner-up clear of c*: the subgradient is unique
        assert float(m.detach().abs().min()) >= 1e-6 and float((top2[:, 0] - top2[:, 1]).detach().min()) >= 1e-6
        loss = torch.relu(m).sum()
        loss.backward()
        assert abs(float(loss.detach()) - out["loss"][b]) <= 1e-12 * max(1.0, abs(float(loss.detach())))
        assert np.array_equal(z.grad.numpy(), out["dlogits"][b, :tb].astype(np.float64))
        assert (out["dlogits"][b, tb:] == 0).all()
        assert np.array_equal(out["margins"][b], m.detach().numpy())
    neg = AR.align_margin(logits, labels, BLANK, kappa, -1.0, frames)
    assert np.array_equal(neg["dlogits"], -out["dlogits"]) and np.array_equal(neg["loss"], out["loss"])


def test_zero_loss_is_greedy_decode_equals_target():
    """All margins non-positive at kappa = 0 <=> pi wins every frame's argmax <=> the greedy decode collapses to the labels."""
    T, V = 12, 6
    pi = np.asarray([0, 2, 2, 0, 2, 3, 3, 0, 0, 1, 0, 0])
    z = np.full((T, V), -1.0, dtype=np.float32)
    z[np.arange(T), pi] = 1.0
    row = np.asarray([2, 2, 3, 1], dtype=np.int32)
    out = AR.align_margin(z[None], row[None], BLANK, 0.0)
    assert out["loss"][0] == 0.0 and not out["dlogits"].any() and out["align"][0].tolist() == pi.tolist()
    assert _collapse(np.argmax(z, axis=1)) == row.tolist()
    out = AR.align_margin(z[None], row[None], BLANK, 2.5)                       # margin 2 < kappa: every frame active
    assert out["loss"][0] == pytest.approx(T * 0.5) and (np.abs(out["dlogits"]).sum(axis=2) == 2).all()


# ---- flags and mode rules -----------------------------------------------------------------------------------------------------
def _args(**over):
    from paa_amd import attack_clips
    a = attack_clips.create_arg_parser().parse_args([])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_parser_defaults_and_choices():
    from paa_amd import attack_clips
    from paa_amd.training_utils import parser
    for make in (parser.create_arg_parser, attack_clips.create_arg_parser):
        a = make().parse_args([])
        assert (a.loss_type, a.margin_kappa) == ("ctc", 1.0)
        a = make().parse_args(["--loss_type", "margin", "--margin_kappa", "0.25"])
        assert (a.loss_type, a.margin_kappa) == ("margin", 0.25)
        with pytest.raises(SystemExit):
            make().parse_args(["--loss_type", "hinge"])


def test_modes_record_and_defaults():
    from paa_amd.training_utils.modes import MARGIN, RULES, Modes, check
    m = Modes.of()
    assert (m.loss_type, m.kappa, m.margin_on) == ("ctc", 1.0, False)
    m = Modes.of(_args(loss_type="margin", margin_kappa=0.5, attack_mode="targeted"))
    assert (m.loss_type, m.kappa, m.margin_on, m.targeted) == ("margin", 0.5, True, True)
    check(m, MARGIN)
    check(Modes.of(_args(loss_type="margin", margin_kappa=0.0, attack_mode="targeted")), MARGIN)
    # with the default flags neither rule is looked at, whatever kappa holds
    check(Modes.of(_args()), MARGIN)
    check(Modes.of(_args(margin_kappa=-3.0)), MARGIN)
    assert MARGIN == ("margin_untargeted", "margin_kappa") and all(RULES[k].mode == "margin_on" for k in MARGIN)


@pytest.mark.parametrize("flags,key,msg", [
    (dict(attack_mode="untargeted"), "margin_untargeted", "--loss_type margin needs --attack_mode targeted: the hinge is flat"),
    (dict(attack_mode="targeted", margin_kappa=-0.5), "margin_kappa", "margin_kappa must be finite and >= 0, got -0.5"),
    (dict(attack_mode="targeted", margin_kappa=float("nan")), "margin_kappa", "margin_kappa must be finite and >= 0, got nan"),
    (dict(attack_mode="targeted", margin_kappa=float("inf")), "margin_kappa", "margin_kappa must be finite and >= 0, got inf"),
])
def test_margin_refusals_by_rule_message_and_entry_point(flags, key, msg):
    import torch
    from paa_amd import attack_clips, run_attack
    from paa_amd.training_utils import modes
    a = _args(loss_type="margin", norm_type="snr", **flags)
    m = modes.Modes.of(a)
    assert modes.RULES[key].exc is ValueError and modes.RULES[key].when(m, modes.Ctx())
    with pytest.raises(ValueError, match=re.escape(msg)):
        modes.check(m, (key,))
    assert [k for k in modes.MARGIN if modes.RULES[k].when(m, modes.Ctx())][0] == key
    # both entry points raise it with their flag rules, before anything touches a GPU
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "is_available", lambda: False)
        with pytest.raises(ValueError, match=re.escape(msg)):
            attack_clips.main(a)
        mp.setattr(torch.cuda, "is_available", lambda: True)
        with pytest.raises(ValueError, match=re.escape(msg)):
            run_attack.main(a)


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
    assert len(lib._SIGS["paa_align_margin"][1]) == 18 and len(lib._SIGS["paa_model_set_loss"][1]) == 3
    assert L.paa_align_margin_work_floats(3, 1499, 32, 450) % 4 == 0 and L.paa_align_margin_work_floats(0, 7, 5, 2) == 0
