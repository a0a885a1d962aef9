"""The playback chain (DESIGN.md "The playback chain"): what lies between the universal perturbation and the recogniser,

    place (place.py, §6f) -> drift (channel.py, §6k) -> rooms (rir.py, §6g) -> + noise (channel.py)

— drift belongs to the emitter, the room to the path, noise to the microphone — and the adjoints in reverse order on the way back.
``Site`` (site.py) is what the three links share on the host: the identity of their draws (seed, stream, global clip id), the step
counter on the device, and the pinning of explicit values.  ``PlaybackChain`` holds the sites of one place where the chain runs
(the training step, or one evaluation) and orders their launches.  ``check`` / ``check_flags`` / ``suffix`` / ``results_extra`` are the three
links' own, in the chain's order: the order decides which refusal wins (modes.py).

``ClipChain`` is the same chain for per-clip perturbations: what enters is the mixture a_r (x_b + delta_b), G draws
per clip, and the gradient rows of a clip's draws are summed into that clip's row.  The links between the two ends, and their order,
are ``PlaybackChain._links`` / ``_links_back`` for both.
"""
from __future__ import annotations

import torch

from .. import _lib
from . import channel, place, rir
from .modes import Modes
from .site import Site  # noqa: F401  (chain.Site)


class PlaybackChain:
    """The rows the model sees at one site with placement, room responses and / or the playback channel on: a ``place.Placer``,
    with room responses on a ``rir.Reverb``, with the channel on a ``channel.Channel``, all keyed by ``rir.draw_seed`` and the global
    clip id ``rank * max_batch + b``.  With placement off the rows are placed at explicit zero shifts and unit gains, and nothing is
    drawn for them."""

    def __init__(self, args, model, Lp: int, stream_id: int, with_grad: bool = True, rank: int = 0, L=None):
        nb = int(model.max_batch)
        self._sites(args, model.device, nb, int(model.length if L is None else L), int(Lp), stream_id, with_grad, rank * nb,
                    place.shift_on(args))

    def _sites(self, args, dev, nb, L, Lp, stream_id, with_grad, clip_base, shift):
        """The three link objects for ``nb`` rows of L samples, the first of global id ``clip_base``."""
        m, seed = Modes.of(args), rir.draw_seed(args)
        self.placer = place.Placer(dev, nb, L, Lp, seed, stream_id, shift, place.gain_db(args), clip_base=clip_base,
                                   with_grad=with_grad)
        if not m.place_on:
            self.placer.set_placement([0] * nb)
        self.reverb = rir.Reverb(dev, rir.bank_of(args), nb, L, seed, stream_id, clip_base=clip_base,
                                 with_grad=with_grad) if m.rir_on else None
        self.chan = channel.Channel(dev, nb, L, seed, stream_id, m.drift_ppm, m.noise_snr, clip_base=clip_base,
                                    with_grad=with_grad) if m.chan_on else None
        self._on = [s for s, on in ((self.placer, m.place_on), (self.reverb, m.rir_on), (self.chan, m.chan_on)) if on]

    @property
    def clip_base(self):
        """Global id of this rank's first clip in every site's draws; assignable per step."""
        return self.placer.clip_base

    @clip_base.setter
    def clip_base(self, v):
        for s in (self.placer, self.reverb, self.chan):
            if s is not None:
                s.clip_base = int(v)

    def counters(self):
        """The device counters of the sites whose mode is on: place, rooms, channel draw, channel noise."""
        return [c for s in self._on for c in s.counters()]

    def set_step(self, n: int):
        """Every such counter to ``n`` (a resumed run goes on drawing where the epochs before it stopped)."""
        for s in self._on:
            s.set_step(n)

    def rows(self, p, B: int, clean=None):
        """draw -> rows [-> channel draw -> drift] [-> room draw -> rows through the rooms] [-> + noise]; an explicit placement /
        explicit channels / explicit rooms skip their draw.  ``clean`` (B, L): the clean batch, whose level scales the noise."""
        pl = self.placer
        if not pl.explicit:
            pl.draw(B)
        return self._links(pl.place(p, B), pl.rows, B, clean)      # the whole buffer the last launch wrote, and its first B rows

    def _links(self, rows, buf, B: int, clean):
        """The links behind the first end, in the chain's order: ``buf`` is the whole buffer the last launch wrote, ``rows`` its
        first B.  The one place that orders them, for every chain."""
        rv, ch = self.reverb, self.chan
        if ch is not None:
            if not ch.explicit:
                ch.draw(B)
            if ch.drift_on:
                rows, buf = ch.apply(buf, B), ch.rows
        if rv is not None:
            if not rv.explicit:
                rv.draw(B)
            rows, buf = rv.apply(buf, B), rv.rows
        if ch is not None and ch.noise_on:
            if clean is None:
                raise ValueError("ambient noise (noise_snr_db) needs the clean batch: rows(p, B, clean)")
            ch.add_noise(buf, clean, B)
        return rows

    def reduce(self, B: int, grad):
        """The model's gradient rows (``placer.grad_rows``) [-> the rooms' adjoint] [-> the drift's transpose] -> adjoint gather-sum
        into ``grad``.  Noise does not depend on the perturbation: the backward pass does not see it."""
        pl = self.placer
        g = self._links_back(B)
        pl.reduce(B, grad, None if g is pl.grad_rows else g)

    def _links_back(self, B: int):
        """The adjoints of ``_links`` in reverse order on ``placer.grad_rows`` -> the gradient rows the first end's adjoint reads."""
        rv, ch = self.reverb, self.chan
        g = self.placer.grad_rows
        if rv is not None:
            g = rv.adjoint(g, B)
        if ch is not None and ch.drift_on:
            g = ch.adjoint(g, B)
        return g


class ClipChain(PlaybackChain):
    """The chain of per-clip perturbations: B clips, G draws each, R = B * G rows, r = b * G + g.  The same link
    objects, sized R, and the same ordering code; only the two ends differ — what enters is the mixture a_r * (x_b + delta_b)
    (``paa_eot_rows``: one loudspeaker plays the adversarial example) and the gradient rows of a clip's draws are summed into that
    clip's row (``paa_eot_reduce``).  The ``Placer`` draws the gains only (shift off) and lends its row buffers.  ``clip_base`` is
    the global id of row 0: G * (global index of the batch's first clip)."""

    def __init__(self, args, dev, max_rows: int, L: int, draws: int, stream_id: int, with_grad: bool = True, clip_base: int = 0):
        self.G, self.max_rows, self.L = int(draws), int(max_rows), int(L)
        if self.G < 1 or self.max_rows < self.G:
            raise ValueError(f"{self.G} draws per clip need a model of at least that many rows, got max_batch {self.max_rows}")
        self._sites(args, dev, self.max_rows, self.L, self.L, stream_id, with_grad, clip_base, False)
        noise = self.chan is not None and self.chan.noise_on
        self.clean_rows = self.placer._zeros() if noise else None          # x_b per row: the level reference of the noise

    def rows(self, delta, B: int, clean):
        """delta, clean (B, L) -> the R rows the model hears (gain draw -> a_r (x_b + delta_b) -> the links)."""
        pl, R = self.placer, B * self.G
        pl._fits(R)
        if not pl.explicit:
            pl.draw(R)
        with torch.cuda.device(pl.dev):
            _lib.check(_lib.lib().paa_eot_rows(_lib.ptr(clean), _lib.ptr(delta), _lib.ptr(pl.gain), _lib.ptr(pl.rows),
                                               _lib.ptr(self.clean_rows), B, self.G, self.L, _lib.stream_ptr()))
        return self._links(pl.rows[:R], pl.rows, R, self.clean_rows)

    def reduce(self, B: int, grad):
        """``placer.grad_rows`` (R, L) -> the links' adjoints -> grad (B, L): row b the sum over clip b's draws."""
        pl = self.placer
        if grad.numel() != B * self.L:
            raise ValueError(f"gradient buffer holds {grad.numel()} floats, expected {B} x {self.L}")
        g = self._links_back(B * self.G)
        with torch.cuda.device(pl.dev):
            _lib.check(_lib.lib().paa_eot_reduce(_lib.ptr(g), _lib.ptr(pl.gain), _lib.ptr(grad), B, self.G, self.L,
                                                 _lib.stream_ptr()))


def check(args, L: int, Lp: int, eager_adam: bool = False) -> None:
    """What the chain's modes do not combine with, for clips of L and a perturbation of Lp samples; raises before any launch or
    collective."""
    place.check(args, L, Lp, eager_adam)
    rir.check(args, eager_adam)
    channel.check(args, eager_adam)


def check_flags(args) -> None:
    """The refusals that need no length and no stepper."""
    place.check_flags(args)
    rir.check_flags(args)
    channel.check_flags(args)


def suffix(args) -> str:
    """Run-directory part of the modes that are on; empty with all off."""
    return place.suffix(args) + rir.suffix(args) + channel.suffix(args)


def results_extra(args, Lp: int) -> dict:
    """results.json keys of the modes that are on."""
    return {**place.results_extra(args, Lp), **rir.results_extra(args), **channel.results_extra(args)}
