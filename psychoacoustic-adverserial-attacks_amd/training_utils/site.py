"""``Site``: what the links of the playback chain (chain.py; place.py, rir.py, channel.py) share on the host."""
from __future__ import annotations

import torch


class Site:
    """Fixed identity of one link's draws at one site: Philox key ``seed``, ``stream_id`` (place.STREAM_TRAIN / STREAM_EVAL), the
    global id ``clip_base`` of the first clip, and the step ``counter`` on the device that every draw reads and advances, so that a
    captured step draws anew on every replay.  ``explicit``: values pinned by the link's ``set_*`` stand in for the draw."""

    def __init__(self, dev, max_batch: int, L: int, seed: int, stream_id: int, clip_base: int = 0):
        self.dev, self.max_batch, self.L = dev, int(max_batch), int(L)
        self.seed, self.stream_id, self.clip_base = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id), int(clip_base)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.explicit = False

    def _zeros(self):
        return torch.zeros(self.max_batch, self.L, dtype=torch.float32, device=self.dev)

    def _fits(self, B):
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"batch {B} outside [1, {self.max_batch}]")

    def _base(self, clip_base):
        return self.clip_base if clip_base is None else int(clip_base)

    def _check_rows(self, t, B, name="rows"):
        if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < B * self.L:
            raise ValueError(f"{name} must be contiguous float32 with at least {B} x {self.L} elements")

    def counters(self):
        """The device counters a step of this site advances."""
        return [self.counter]

    def set_step(self, n: int):
        """Step counter(s) of the next draw (resume, tests); stream-ordered."""
        for c in self.counters():
            c.fill_(int(n))

    def unpin(self):
        """Back to drawing: what ``set_placement(None)`` / ``set_rooms(None)`` / ``set_channel(None)`` do."""
        self.explicit = False
