"""Random placement of the universal perturbation: delta has Lp samples, the clips L, and clip b sees

    rows[b][i] = a_b * delta[(i + s_b) mod Lp]            shift s_b in [0, Lp), gain a_b > 0

— a circular shift (Lp = L), a tiling (Lp < L; the seam is not smoothed, and a room response laid over the rows
(training_utils/rir.py) convolves linearly across it, not circularly) or a window (Lp > L) of delta, at a playback level of its own.  The gradient of delta is the adjoint, a gather-sum over the per-clip gradient rows.  The three launches
(``paa_place_draw`` / ``paa_place_rows`` / ``paa_place_reduce``) allocate nothing and the draw's step counter lives on the device,
so a captured step draws anew on every replay.

Flags (training_utils/parser.py): ``--perturbation_seconds`` (None = the clip length), ``--place_shift {none,random}``,
``--place_gain_db G`` (gain uniform in [-G, +G] dB).  Placement is ON iff perturbation_seconds is set, place_shift == "random" or
place_gain_db > 0; OFF leaves every caller exactly as it was.
"""
from __future__ import annotations

import logging
from dataclasses import replace

import torch

from .. import _lib
from . import modes
from .modes import Ctx, Modes
from .site import Site

logger = logging.getLogger(__name__)

STREAM_TRAIN, STREAM_EVAL = 0, 1
_FREQ_NORMS = ("fletcher_munson", "min_max_freqs", "max_phon")
_hop_warned = set()


def placement_on(args) -> bool:
    return Modes.of(args).place_on


def shift_on(args) -> bool:
    return modes.check(replace(Modes.of(args), place_on=True), ("shift_range",)).shift_on


def gain_db(args) -> float:
    return modes.check(replace(Modes.of(args), place_on=True), ("gain_range",)).gain_db


def perturbation_length(args, clip_length: int) -> int:
    """Lp: round(perturbation_seconds * sr), or the clip length when the flag is not set."""
    s = getattr(args, "perturbation_seconds", None)
    if s is None:
        return int(clip_length)
    lp = int(round(float(s) * int(args.sr)))
    if lp < 1:
        raise ValueError(f"perturbation_seconds {s} gives a perturbation of {lp} samples")
    return lp


def check_flags(args) -> None:
    """The refusals that need no length: flag values outside their ranges, and the masking norm / masking loss.  A no-op with
    placement off."""
    modes.check(Modes.of(args), modes.PLACE_FLAGS)


def check(args, L: int, Lp: int, eager_adam: bool = False) -> None:
    """What placement does not combine with, for clips of L and a perturbation of Lp samples; raises before any launch or
    collective.  A no-op with placement off."""
    m = modes.check(Modes.of(args), modes.PLACE, Ctx(1, eager_adam, L, Lp))
    hop = int(getattr(args, "hop_length", 256))
    if m.place_on and Lp % hop and any(n in _FREQ_NORMS for n in m.norms) and (Lp, hop) not in _hop_warned:
        _hop_warned.add((Lp, hop))
        logger.warning("perturbation length %d is no multiple of hop_length %d: the frequency-domain projection zeroes its last %d "
                       "samples every step", Lp, hop, Lp % hop)


def suffix(args) -> str:
    """Run-directory part of a run with placement: "_place<Lp samples>[s][g<G>]"; empty with placement off, so other runs keep
    their directory (and resume from it)."""
    if not placement_on(args):
        return ""
    s = getattr(args, "perturbation_seconds", None)
    out = "_place" + (f"{perturbation_length(args, 0)}" if s is not None else "")
    if shift_on(args):
        out += "s"
    if gain_db(args) > 0:
        out += f"g{gain_db(args):g}"
    return out


def results_extra(args, Lp: int) -> dict:
    """results.json keys of a run with placement (none otherwise)."""
    if not placement_on(args):
        return {}
    return {"perturbation_length": int(Lp), "place_shift": str(Modes.of(args).place_shift), "place_gain_db": gain_db(args)}


class Placer(Site):
    """Fixed device buffers and the three launches of one placement site (the training step, or one evaluation).
    ``draw`` -> shift / gain of the next step's clips (the placement stream of csrc/philox.h), ``place`` -> rows[:B], ``reduce`` ->
    the adjoint of ``place`` on grad_rows[:B]."""

    def __init__(self, dev, max_batch: int, L: int, Lp: int, seed: int, stream_id: int, shift: bool, gain_db_: float,
                 clip_base: int = 0, with_grad: bool = True):
        super().__init__(dev, max_batch, L, seed, stream_id, clip_base)
        self.Lp, self.shift_on, self.gain_db = int(Lp), bool(shift), float(gain_db_)
        self.shift = torch.zeros(self.max_batch, dtype=torch.int32, device=dev)
        self.gain = torch.ones(self.max_batch, dtype=torch.float32, device=dev)
        self.rows = self._zeros()
        self.grad_rows = self._zeros() if with_grad else None

    def set_placement(self, shift, gain=None):
        """Pin explicit shifts (and gains, default 1) for the clips of the following steps by a stream-ordered copy: the draw is
        skipped until ``set_placement(None)``.  Which of the two a captured graph holds is fixed by ``capture()``."""
        if shift is None:
            return self.unpin()
        s = torch.as_tensor(shift, dtype=torch.int32).reshape(-1)
        g = torch.ones(s.numel(), dtype=torch.float32) if gain is None else torch.as_tensor(gain, dtype=torch.float32).reshape(-1)
        self._fits(s.numel())
        if g.numel() != s.numel():
            raise ValueError(f"{s.numel()} shifts but {g.numel()} gains")
        if not bool((g > 0).all()):
            raise ValueError("gains must be > 0")
        self.shift[: s.numel()].copy_(s, non_blocking=True)
        self.gain[: g.numel()].copy_(g, non_blocking=True)
        self.explicit = True

    def draw(self, B: int, clip_base=None):
        self._fits(B)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_place_draw(self.seed, _lib.ptr(self.counter), self.stream_id, self._base(clip_base), B,
                                                 self.Lp, int(self.shift_on), self.gain_db, _lib.ptr(self.shift),
                                                 _lib.ptr(self.gain), _lib.stream_ptr()))

    def place(self, p, B: int):
        self._fits(B)
        if p.numel() != self.Lp:
            raise ValueError(f"Loaded perturbation length {p.numel()} != expected {self.Lp}")
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_place_rows(_lib.ptr(p), self.Lp, _lib.ptr(self.shift), _lib.ptr(self.gain),
                                                 _lib.ptr(self.rows), B, self.L, _lib.stream_ptr()))
        return self.rows[:B]

    def reduce(self, B: int, grad, grad_rows=None):
        """``grad_rows``: gradient rows to reduce instead of this site's own (rir.Reverb.adjoint's)."""
        self._fits(B)
        if grad.numel() != self.Lp:
            raise ValueError(f"gradient buffer holds {grad.numel()} floats, expected {self.Lp}")
        src = self.grad_rows if grad_rows is None else grad_rows
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_place_reduce(_lib.ptr(src), _lib.ptr(self.shift), _lib.ptr(self.gain),
                                                   _lib.ptr(grad), B, self.L, self.Lp, _lib.stream_ptr()))


def place_rows(p, L: int, shift=None, gain=None, B: int = 1):
    """rows (B, L) of the perturbation ``p`` (Lp samples, on the GPU) at explicit shifts / gains (default: shift 0, gain 1 — how a
    saved perturbation is laid over an example clip).  Allocates; for files and tests, not for the step."""
    p = p.detach().reshape(-1)
    s = torch.zeros(B, dtype=torch.int32) if shift is None else torch.as_tensor(shift, dtype=torch.int32).reshape(-1)
    pl = Placer(p.device, s.numel(), L, p.numel(), 0, STREAM_EVAL, False, 0.0, with_grad=False)
    pl.set_placement(s, gain)
    return pl.place(p.to(torch.float32).contiguous(), s.numel())
