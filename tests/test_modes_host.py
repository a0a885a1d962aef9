"""No-GPU check of training_utils/modes.py: for every point of a grid of mode flags, each of the five entry points raises exactly what
it raised before the refusals were gathered into one table (tests/golden/mode_refusals.json, recorded with this module's own
``outcomes`` on the commit the fixture names).  The entry points themselves run — run_attack.main, train_epoch, PgdStepper,
evaluation._PlacedEval and attack_clips.main — each up to the first thing it does after its refusals, which is patched to stop it."""
import copy
import itertools
import json
import os
import types

import pytest
import torch

GRID = {
    "norm_type": ["linf", "snr", "fletcher_munson", "masking", "l2+masking"],
    "masking_loss_alpha": [0.0, 0.5],
    "perturbation_seconds": [None, 0.5],
    "place_shift": ["none", "random"],
    "place_gain_db": [0.0, 6.0],
    "rir_bank": ["none", "synthetic"],
    "clip_lengths": ["padded", "true"],
    "world": [1, 2],
    "eager_adam": [False, True],
}
# flag values outside their ranges, as a hand-built namespace brings them: each crossed with EXTRA_GRID
EXTRAS = [
    {"place_gain_db": 21.0},
    {"place_shift": "always", "place_gain_db": 1.0},
    {"rir_bank": "synthetic", "rir_count": 0},
    {"rir_bank": "/no_such_bank.npy"},
    {"rir_bank": "synthetic", "rir_count": 0, "place_shift": "random"},
    {"rir_bank": "synthetic", "place_shift": "always"},
    {"rir_bank": "synthetic", "place_gain_db": -1.0},
]
EXTRA_GRID = {"norm_type": ["linf", "masking"], "clip_lengths": ["padded", "true"], "world": [1, 2], "eager_adam": [False, True]}
ENTRIES = ["runner", "train_epoch", "stepper", "evaluation", "per_clip"]
L = 16000
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mode_refusals.json")


class _Reached(Exception):
    """The entry point got past its refusals."""


def _stop(*a, **kw):
    raise _Reached


def points():
    for v in itertools.product(*GRID.values()):
        yield dict(zip(GRID, v))
    for extra in EXTRAS:
        for v in itertools.product(*EXTRA_GRID.values()):
            yield {**dict(zip(EXTRA_GRID, v)), **extra}


def outcomes(mp):
    """[[outcome per entry] per grid point]: "none", or "<exception class>: <message>".  ``mp``: a pytest.MonkeyPatch."""
    from paa_amd import attack_clips, run_attack
    from paa_amd.training_utils import build, evaluation, pgd, place, rir, train
    world = [1]
    model = types.SimpleNamespace(device=torch.device("cpu"), max_batch=2, length=L, lengths_on=False)
    mp.setattr(torch.distributed, "is_initialized", lambda: world[0] > 1)
    mp.setattr(torch.distributed, "get_world_size", lambda group=None: world[0])
    mp.setattr(torch.distributed, "get_rank", lambda group=None: 0)
    mp.setattr(torch.cuda, "set_device", _stop)             # run_attack.main with several ranks: the process-group start
    mp.setattr(build, "create_logger", _stop)               # ... with one rank: the first call after the pre-check
    mp.setattr(train, "PgdStepper", _stop)                  # train_epoch up to the construction of the stepper
    mp.setattr(pgd._StepperCore, "__init__", _stop)         # PgdStepper.__init__ up to the shared core

    def runner(args, pt, Lp):
        mp.setattr(torch.cuda, "is_available", lambda: True)
        mp.setenv("WORLD_SIZE", str(pt["world"]))
        mp.setenv("RANK", "0")
        run_attack.main(args)

    def train_epoch(args, pt, Lp):
        p = torch.nn.Parameter(torch.zeros(1, Lp))          # an optimizer the device step does not cover takes the eager route
        opt = torch.optim.Adam([p], lr=0.1, weight_decay=0.1 if pt["eager_adam"] else 0.0)
        train.train_epoch(args, [], p, model, 0, None, None, None, None, opt)

    def stepper(args, pt, Lp):
        pgd.PgdStepper(model, args, L, p_length=Lp)

    def evaluation_(args, pt, Lp):
        if place.placement_on(args) or rir.rir_on(args):    # evaluate(perturbed=True)
            evaluation._PlacedEval(args, model, torch.zeros(1, Lp))

    def per_clip(args, pt, Lp):
        mp.setattr(torch.cuda, "is_available", lambda: False)          # main leaves right after its refusals
        attack_clips.main(args)

    base = attack_clips.create_arg_parser().parse_args([])
    base.rir_count, base.rir_taps, base.optimizer_type = 2, 16, "adam"
    out = []
    for pt in points():
        world[0] = pt["world"]
        row = []
        for f in (runner, train_epoch, stepper, evaluation_, per_clip):
            args = copy.copy(base)
            for k, v in pt.items():
                if k not in ("world", "eager_adam"):
                    setattr(args, k, v)
            try:
                f(args, pt, place.perturbation_length(args, L))
                got = "none"
            except (_Reached, SystemExit):
                got = "none"
            except Exception as e:      # noqa: BLE001
                got = f"{type(e).__name__}: {e}"
            row.append(got)
        out.append(row)
    return out


def test_every_entry_point_refuses_what_it_refused():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["grid"] == GRID and fx["extras"] == EXTRAS and fx["extra_grid"] == EXTRA_GRID and fx["entries"] == ENTRIES and fx["L"] == L
    want = [[fx["messages"][i] for i in row] for row in fx["cases"]]
    # the fixture is no vacuous one: every entry raises and passes, and every refusal sentence of the recorded commit's place.py,
    # rir.py, pgd.py and train.py (fx["required"], copied from its source when the fixture was recorded) is raised somewhere
    for e, name in enumerate(ENTRIES):
        col = [row[e] for row in want]
        assert "none" in col and any(c != "none" for c in col), name
    assert len(fx["required"]) == 19
    for msg in fx["required"]:
        assert msg in fx["messages"], msg
    with pytest.MonkeyPatch.context() as mp:
        got = outcomes(mp)
    assert len(got) == len(want)
    bad = [(pt, ENTRIES[e], g[e], w[e]) for pt, g, w in zip(points(), got, want) for e in range(len(ENTRIES)) if g[e] != w[e]]
    assert not bad, f"{len(bad)} of {len(want) * len(ENTRIES)} cases differ; the first: {bad[0]}"
