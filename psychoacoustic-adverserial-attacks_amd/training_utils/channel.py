"""The playback channel on the placement layer: what lies between the emitter and the recogniser besides the place
(place.py, §6f) and the room (rir.py, §6g).

    drift   y_b[i] = sum_{t=-7..8} w(t - f) x_b[n + t],  n + f = i * r_b       the emitter's clock runs at r_b times the recorder's
    noise   rows_b[i] += sigma_b * z_{b,i},  sigma_b = rms(clean_b) * 10^(-snr_b / 20)       the microphone's own noise

with r_b = rq_b / 2^32 uniform in 1 +- drift_ppm * 1e-6 and snr_b uniform in [LO, HI] dB, both drawn per clip and per step, w a
16-tap Hann-windowed sinc (no band-limiting for r > 1: meant for |r - 1| <= 0.1) and z a standard normal drawn anew in every
step.  The chain of a step is place -> drift -> rooms -> + noise: drift belongs to the emitter, the room to the path, noise to the
microphone.  The gradient takes the exact transpose of the drift between the rooms' adjoint and ``paa_place_reduce``; noise does
not depend on delta and the backward pass does not see it.  The launches (``paa_chan_draw`` / ``paa_drift_apply`` /
``paa_noise_add``) allocate nothing and both step counters — the draw's and the noise's own — live on the device, so a captured
step draws anew on every replay, and pinned channels (``set_channel``) still hear fresh noise.

Flags (training_utils/parser.py): ``--drift_ppm P`` (0 = off), ``--noise_snr_db LO HI`` (absent = off).  The mode is ON iff
drift_ppm > 0 or noise_snr_db is set; OFF leaves every caller exactly as it was.
"""
from __future__ import annotations

import torch

from .. import _lib
from . import modes
from .modes import Ctx, Modes
from .site import Site

Q32 = 1 << 32
RQ_MIN, RQ_MAX = 1 << 31, 1 << 33          # the device clamps a ratio to [0.5, 2]


def chan_on(args) -> bool:
    return Modes.of(args).chan_on


def check_flags(args) -> None:
    """The refusals that need no stepper: flag values outside their ranges, the masking norm / loss."""
    modes.check(Modes.of(args), modes.CHANNEL_FLAGS)


def check(args, eager_adam: bool = False) -> None:
    """What the mode does not combine with; raises before any launch or collective.  With the mode off only the ranges are read."""
    modes.check(Modes.of(args), modes.CHANNEL, Ctx(1, eager_adam))


def refuse_for_clips(args) -> None:
    """paa_amd.attack_clips: the channel of per-clip perturbations is not part of this."""
    modes.check(Modes.of(args), ("chan_range", "chan_clips"))


def drift_q32(ppm: float) -> int:
    """D = round(drift_ppm * 1e-6 * 2^32): the draw's half-width in Q32, computed here on the host."""
    return int(round(float(ppm) * 1e-6 * float(Q32)))


def rq_of(ratio) -> int:
    """The Q32 integer of a float ratio, clamped as the device clamps it."""
    return min(max(int(round(float(ratio) * float(Q32))), RQ_MIN), RQ_MAX)


def suffix(args) -> str:
    """Run-directory part of a run with the mode on: "_drift<ppm>" and / or "_noise<lo>-<hi>"; empty with it off."""
    m = modes.check(Modes.of(args), ("chan_range",))
    out = f"_drift{m.drift_ppm:g}" if m.drift_on else ""
    if m.noise_on:
        out += f"_noise{m.noise_snr[0]:g}-{m.noise_snr[1]:g}"
    return out


def results_extra(args) -> dict:
    """results.json keys of a run with the mode on (none otherwise)."""
    m = modes.check(Modes.of(args), ("chan_range",))
    out = {"drift_ppm": float(m.drift_ppm)} if m.drift_on else {}
    if m.noise_on:
        out["noise_snr_db"] = [float(m.noise_snr[0]), float(m.noise_snr[1])]
    return out


class Channel(Site):
    """Fixed device buffers and the launches of one channel site (the training step, or one evaluation), beside ``place.Placer``
    and ``rir.Reverb``.  ``draw`` -> (rq, snr_db) of the next step's clips (the channel stream of csrc/philox.h); ``apply`` ->
    rows[:B] = the drifted input; ``adjoint`` -> grad_rows[:B] = the transpose of ``apply`` on gradient rows; ``add_noise`` -> in
    place on the rows it is given, samples keyed by (``noise_counter``, clip, sample), a counter of the noise's own (the noise
    stream); ``set_step`` sets both."""

    def __init__(self, dev, max_batch: int, L: int, seed: int, stream_id: int, drift_ppm: float = 0.0, noise_snr=None,
                 clip_base: int = 0, with_grad: bool = True):
        super().__init__(dev, max_batch, L, seed, stream_id, clip_base)
        m = modes.check(Modes.of(drift_ppm=drift_ppm, noise_snr_db=noise_snr), ("chan_range",))
        self.drift_on, self.noise_on = m.drift_on, m.noise_on
        self.D = drift_q32(m.drift_ppm)
        self.snr_lo, self.snr_hi = (float(m.noise_snr[0]), float(m.noise_snr[1])) if m.noise_on else (0.0, 0.0)
        self.rq = torch.full((self.max_batch,), Q32, dtype=torch.int64, device=dev)          # the device reads it as uint64
        self.snr_db = torch.zeros(self.max_batch, dtype=torch.float32, device=dev)
        self.sigma = torch.zeros(self.max_batch, dtype=torch.float32, device=dev)
        self.noise_counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rows = self._zeros() if self.drift_on else None
        self.grad_rows = self._zeros() if self.drift_on and with_grad else None

    def counters(self):
        return [self.counter, self.noise_counter]

    def set_channel(self, ratio, snr_db=None):
        """Pin explicit ratios (floats, or Q32 integers in an integer tensor / list of ints) and SNRs (default: what the buffer
        holds) for the clips of the following steps by a stream-ordered copy: the draw is skipped until ``set_channel(None)``.  The
        noise keeps its own counter and stays fresh.  Which of the two a captured graph holds is fixed by ``capture()``."""
        if ratio is None:
            return self.unpin()
        r = ratio.reshape(-1).tolist() if isinstance(ratio, torch.Tensor) else list(ratio)          # Python floats: no float32 detour
        q = torch.tensor([int(x) if isinstance(x, int) else int(round(float(x) * float(Q32))) for x in r], dtype=torch.int64)
        self._fits(q.numel())
        if bool(((q < RQ_MIN) | (q > RQ_MAX)).any()):
            raise ValueError(f"ratios must lie in [0.5, 2] (Q32 in [{RQ_MIN}, {RQ_MAX}])")
        self.rq[: q.numel()].copy_(q, non_blocking=True)
        if snr_db is not None:
            s = torch.as_tensor(snr_db, dtype=torch.float32).reshape(-1)
            if s.numel() != q.numel():
                raise ValueError(f"{q.numel()} ratios but {s.numel()} SNRs")
            self.snr_db[: s.numel()].copy_(s, non_blocking=True)
        self.explicit = True

    def draw(self, B: int, clip_base=None):
        self._fits(B)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_chan_draw(self.seed, _lib.ptr(self.counter), self.stream_id, self._base(clip_base), B, self.D,
                                                self.snr_lo, self.snr_hi, _lib.ptr(self.rq), _lib.ptr(self.snr_db),
                                                _lib.stream_ptr()))

    def _launch(self, src, dst, B, adjoint):
        self._fits(B)
        if dst is None:
            raise RuntimeError("the channel was built with drift off (drift_ppm)" if not self.drift_on else
                               "the channel was built without gradient rows")
        self._check_rows(src, B)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_drift_apply(_lib.ptr(self.rq), _lib.ptr(src), _lib.ptr(dst), B, self.L, adjoint,
                                                  _lib.stream_ptr()))
        return dst[:B]

    def apply(self, rows, B: int):
        """rows (B, L) -> self.rows[:B], every clip at its ratio."""
        return self._launch(rows, self.rows, B, 0)

    def adjoint(self, grad_rows, B: int):
        """Gradient rows (B, L) -> self.grad_rows[:B], the gradient with respect to the rows ``apply`` read."""
        return self._launch(grad_rows, self.grad_rows, B, 1)

    def add_noise(self, rows, clean, B: int, clip_base=None):
        """rows[:B] += sigma_b z, in place; sigma from ``clean`` (B, L) and the SNRs of the last draw / ``set_channel``."""
        self._fits(B)
        self._check_rows(rows, B)
        self._check_rows(clean, B, "clean")
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_noise_add(self.seed, _lib.ptr(self.noise_counter), self.stream_id, self._base(clip_base),
                                                _lib.ptr(clean), _lib.ptr(self.snr_db), _lib.ptr(self.sigma), _lib.ptr(rows), B,
                                                self.L, _lib.stream_ptr()))
        return rows[:B]


def drift(rows, ratio, adjoint: bool = False):
    """``rows`` (B, L, on the GPU) resampled at ``ratio`` (one per row; floats or Q32 integers).  Allocates; for files and tests,
    not for the step."""
    rows = rows.detach().to(torch.float32).contiguous()
    B, L = rows.shape
    ch = Channel(rows.device, B, L, 0, 1, drift_ppm=1.0, with_grad=True)
    ch.set_channel(ratio)
    return ch.adjoint(rows, B) if adjoint else ch.apply(rows, B)


def add_noise(rows, clean, snr_db, seed: int = 0, step: int = 0, stream_id: int = 1, clip_base: int = 0):
    """A copy of ``rows`` (B, L, on the GPU) with noise at ``snr_db`` (one per row) below the level of ``clean``.  Allocates; for
    files and tests, not for the step."""
    rows = rows.detach().to(torch.float32).contiguous().clone()
    B, L = rows.shape
    ch = Channel(rows.device, B, L, seed, stream_id, noise_snr=(0.0, 0.0), clip_base=clip_base, with_grad=False)
    ch.set_channel([1.0] * B, snr_db)
    ch.noise_counter.fill_(int(step))
    return ch.add_noise(rows, clean.detach().to(torch.float32).contiguous(), B)
