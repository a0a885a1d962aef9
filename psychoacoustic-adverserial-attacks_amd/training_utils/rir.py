"""Room responses on the placement layer: clip b of a step hears its placed row through a room,

    rows[b][i] = a_b * delta[(i + s_b) mod Lp]                                (placement; s = 0, a = 1 when placement is off)
    r_b[i]     = sum_{k=0}^{min(K-1, i)} h_{c_b}[k] * rows[b][i - k]          (causal FIR, zero history, the tail beyond L dropped)

with ``h`` a bank (N, K) of float32 room responses on the device and c_b in [0, N) drawn per clip and per step.  The convolution is
linear, not circular, also for a tiled delta.  The gradient takes the exact adjoint before ``paa_place_reduce``.  The two launches
(``paa_rir_draw`` / ``paa_rir_apply``) allocate nothing and the draw's step counter — one of its own, not the placer's — lives on
the device, so a captured step draws anew on every replay.  The projections and norms keep acting on delta itself: the bound holds
for the emitted signal.

Flags (training_utils/parser.py): ``--rir_bank {none,synthetic,PATH}``, ``--rir_count``, ``--rir_taps``, ``--rir_rt60 LO HI``,
``--rir_drr_db``, ``--rir_seed``.  The mode is ON iff rir_bank is not "none"; OFF leaves every caller exactly as it was.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .. import _lib, synth
from . import modes
from .modes import Ctx, Modes
from .site import Site

MAX_TAPS = 16384                      # PAA_RIR_MAX_TAPS of include/paa_hip.h
MAX_COUNT = 65536
_BANKS = {}


def rir_on(args) -> bool:
    return Modes.of(args).rir_on


def _synthetic_flags(args):
    """(N, K, rt60_lo, rt60_hi, drr_db, seed) of a synthetic bank, range-checked."""
    n, k = int(getattr(args, "rir_count", 64)), int(getattr(args, "rir_taps", 4096))
    if not 1 <= n <= MAX_COUNT:
        raise ValueError(f"rir_count must be in [1, {MAX_COUNT}], got {n}")
    if not 1 <= k <= MAX_TAPS:
        raise ValueError(f"rir_taps must be in [1, {MAX_TAPS}], got {k}")
    rt = getattr(args, "rir_rt60", (0.2, 0.6))
    if len(rt) != 2 or not 0.01 <= float(rt[0]) <= float(rt[1]) <= 10.0:
        raise ValueError(f"rir_rt60 must be LO HI with 0.01 <= LO <= HI <= 10 seconds, got {list(rt)}")
    d = float(getattr(args, "rir_drr_db", 6.0))
    if not -40.0 <= d <= 60.0:
        raise ValueError(f"rir_drr_db must be in [-40, 60], got {d}")
    seed = getattr(args, "rir_seed", None)
    seed = int(getattr(args, "seed", 5) if seed is None else seed)
    return n, k, float(rt[0]), float(rt[1]), d, seed


def check_flags(args) -> None:
    """The refusals that need no stepper: flag values outside their ranges, the masking norm / loss.  A no-op with the mode off."""
    check(args)


def check(args, eager_adam: bool = False) -> None:
    """What the mode does not combine with; raises before any launch or collective.  A no-op with the mode off."""
    m = Modes.of(args)
    if m.rir_on:          # the synthetic bank's flags range-checked, or a bank file read and checked, here on the host
        _synthetic_flags(args) if str(args.rir_bank) == "synthetic" else bank_of(args)
    modes.check(m, modes.ROOMS, Ctx(1, eager_adam))


def synthetic_rt60(N: int, rt60_lo: float, rt60_hi: float, seed: int) -> np.ndarray:
    """RT60 of every row of ``synthetic_bank`` in seconds: uniform in [LO, HI] from the repository's counter-based generator."""
    return float(rt60_lo) + (float(rt60_hi) - float(rt60_lo)) * synth.uniform(synth.key_of("rir_rt60", int(seed)), int(N))


def synthetic_bank(N: int, K: int, sr: int, rt60_lo: float, rt60_hi: float, drr_db: float, seed: int) -> np.ndarray:
    """float32 (N, K), computed in float64 on the host from synth.py's generator (Box-Muller normals), so every rank and every
    machine holds the same bits.  Row n: h[0] = 1 (the direct path), h[k] = g_k exp(-3 ln10 k / (rt60_n sr)) for k >= 1 with
    g ~ N(0, 1) — a 60 dB energy decay over rt60_n seconds — the tail then scaled to sum_{k>=1} h[k]^2 = 10^(-drr_db / 10)."""
    N, K = int(N), int(K)
    rt60 = synthetic_rt60(N, rt60_lo, rt60_hi, seed)
    k = np.arange(K, dtype=np.float64)
    out = np.zeros((N, K), dtype=np.float64)
    target = 10.0 ** (-float(drr_db) / 10.0)
    for n in range(N):
        tail = synth.normal(synth.key_of(f"rir{n}", int(seed)), K) * np.exp(-3.0 * math.log(10.0) * k / (rt60[n] * float(sr)))
        tail[0] = 0.0
        e = float(np.sum(tail * tail))
        if e > 0:
            tail *= math.sqrt(target / e)
        out[n] = tail
        out[n, 0] = 1.0
    return out.astype(np.float32)


def load_bank(path: str) -> np.ndarray:
    """A bank from a ``.npy`` or a weights-only ``.pt`` file holding a float (N, K) array; used as it is after the checks."""
    if not os.path.isfile(path):
        raise ValueError(f"rir_bank {path!r}: no such file (none, synthetic, or a .npy / .pt file)")
    if path.endswith(".npy"):
        a = np.load(path, allow_pickle=False)
    elif path.endswith(".pt"):
        t = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"rir_bank {path!r}: holds a {type(t).__name__}, not a tensor")
        a = (t.detach().to(torch.float32) if t.is_floating_point() else t).numpy()
    else:
        raise ValueError(f"rir_bank {path!r}: expected a .npy or .pt file")
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"rir_bank {path!r}: dtype {a.dtype} is not a float type")
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"rir_bank {path!r}: shape {tuple(a.shape)} is not (N, K)")
    if a.shape[1] > MAX_TAPS:
        raise ValueError(f"rir_bank {path!r}: {a.shape[1]} taps, at most {MAX_TAPS}")
    if not np.isfinite(a).all():
        raise ValueError(f"rir_bank {path!r}: holds non-finite values")
    return np.ascontiguousarray(a, dtype=np.float32)


def bank_of(args) -> np.ndarray:
    """The float32 (N, K) bank the flags name, on the host (cached per flag set: the runner asks for its shape, the stepper and
    every evaluation for its values)."""
    which = str(args.rir_bank)
    if which == "synthetic":
        key = ("synthetic", int(args.sr)) + _synthetic_flags(args)
        if key not in _BANKS:
            n, k, lo, hi, d, seed = key[2:]
            _BANKS[key] = synthetic_bank(n, k, int(args.sr), lo, hi, d, seed)
    else:
        key = ("file", os.path.abspath(which), os.path.getmtime(which) if os.path.isfile(which) else None)
        if key not in _BANKS:
            _BANKS[key] = load_bank(which)
    return _BANKS[key]


def suffix(args) -> str:
    """Run-directory part of a run with the mode on: "_rir<N>x<K>"; empty with it off, so other runs keep their directory."""
    if not rir_on(args):
        return ""
    n, k = bank_of(args).shape
    return f"_rir{n}x{k}"


def results_extra(args) -> dict:
    """results.json keys of a run with the mode on (none otherwise)."""
    if not rir_on(args):
        return {}
    n, k = bank_of(args).shape
    return {"rir_bank": str(args.rir_bank), "rir_count": int(n), "rir_taps": int(k)}


def draw_seed(args) -> int:
    """Philox key of the room draw: placement's (place_seed, default seed); counter word 3 keeps the two streams apart."""
    seed = getattr(args, "place_seed", None)
    return int(getattr(args, "seed", 5) if seed is None else seed)


class Reverb(Site):
    """Fixed device buffers and the launches of one reverberation site (the training step, or one evaluation), beside
    ``place.Placer``.  ``draw`` -> room index of the next step's clips (the room stream of csrc/philox.h, a counter of its own),
    ``apply`` -> rows[:B] = h_c * in, ``adjoint`` -> grad_rows[:B] = the adjoint of ``apply`` on the gradient rows of the model."""

    def __init__(self, dev, bank, max_batch: int, L: int, seed: int, stream_id: int, clip_base: int = 0, with_grad: bool = True):
        super().__init__(dev, max_batch, L, seed, stream_id, clip_base)
        bank = torch.as_tensor(bank)
        if bank.dim() != 2 or not bank.is_floating_point() or not 1 <= bank.shape[1] <= MAX_TAPS:
            raise ValueError(f"a bank is a float (N, K <= {MAX_TAPS}) array, got {bank.dtype} {tuple(bank.shape)}")
        self.bank = bank.to(dev, torch.float32).contiguous()
        self.N, self.K = int(bank.shape[0]), int(bank.shape[1])
        self.index = torch.zeros(self.max_batch, dtype=torch.int32, device=dev)
        self.rows = self._zeros()
        self.grad_rows = self._zeros() if with_grad else None

    def set_rooms(self, index):
        """Pin explicit room indices for the clips of the following steps by a stream-ordered copy: the draw is skipped until
        ``set_rooms(None)``.  Which of the two a captured graph holds is fixed by ``capture()``."""
        if index is None:
            return self.unpin()
        c = torch.as_tensor(index, dtype=torch.int32).reshape(-1)
        self._fits(c.numel())
        self.index[: c.numel()].copy_(c, non_blocking=True)
        self.explicit = True

    def draw(self, B: int, clip_base=None):
        self._fits(B)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_rir_draw(self.seed, _lib.ptr(self.counter), self.stream_id, self._base(clip_base), B, self.N,
                                               _lib.ptr(self.index), _lib.stream_ptr()))

    def _launch(self, src, dst, B, adjoint):
        self._fits(B)
        self._check_rows(src, B)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_rir_apply(_lib.ptr(self.bank), self.N, self.K, _lib.ptr(self.index), _lib.ptr(src),
                                                _lib.ptr(dst), B, self.L, adjoint, _lib.stream_ptr()))
        return dst[:B]

    def apply(self, rows, B: int):
        """rows (B, L) -> self.rows[:B], every clip through its room."""
        return self._launch(rows, self.rows, B, 0)

    def adjoint(self, grad_rows, B: int):
        """The model's gradient rows (B, L) -> self.grad_rows[:B], the gradient with respect to the rows ``apply`` read."""
        return self._launch(grad_rows, self.grad_rows, B, 1)


def reverberate(rows, bank, index):
    """``rows`` (B, L, on the GPU) through the rooms ``index`` of ``bank`` (N, K).  Allocates; for files and tests, not for the
    step."""
    rows = rows.detach().to(torch.float32).contiguous()
    B, L = rows.shape
    rv = Reverb(rows.device, bank, B, L, 0, 1, with_grad=False)
    rv.set_rooms(index)
    return rv.apply(rows, B)
