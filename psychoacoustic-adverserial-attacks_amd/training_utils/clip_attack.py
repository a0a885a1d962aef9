"""Per-clip (per-utterance) attacks: one perturbation row delta_b per clip b, on the device step.

Semantics (a per-clip step on B clips is B independent universal steps at batch 1):

    x~_b = clamp(x_b + delta_b, -1, 1)      loss = sum_b CTC_b (HF reduction='sum')
    g_b  = direction * dloss / ddelta_b     (in eval mode CTC_b depends on delta_b alone)
    delta_b += lr * sign(g_b)   |   torch.optim.Adam over the (B, L) tensor
    delta_b  = perturbation_constraint(delta_b[None], x_b[None], args)   for every norm of args.norm_type, in order

With ``args.masking_loss_alpha`` = alpha > 0 clip b's objective is direction * CTC_b - alpha * l_b(delta_b):
``paa_masking_loss`` with one row per clip subtracts alpha * grad l_b from row b of the gradient right after the backward pass.

One launch sequence per step (``paa_model_fwd_bwd_rows`` -> ``paa_sign_step`` / ``paa_adam_step`` over B*L elements ->
``paa_project_rows`` per norm) and no collective: clips are independent, so ranks never exchange gradients.  Everything else —
the Adam bookkeeping, the masking loss, the device WER counters, the warm-up of ``capture()`` — is ``pgd._StepperCore``'s.

True clip lengths: with ``lengths=`` the model attacks the utterance and then pads, and ``paa_mask_tail_rows``
re-zeroes delta_b[len_b:] after every ``paa_project_rows`` (the sign and Adam updates keep a zero tail: its gradient is zero).

Bound search: with ``search=SearchConfig(...)`` every clip carries a bound scale s_b (1 after ``search_reset``).
``paa_clip_search`` sits between the device WER counters and the update: a clip whose counters say "success" has its delta_b (the
one that entered the step), s_b and the step number kept in ``best`` / ``best_scale`` / ``best_step`` and its s_b shrunk; the
projections then run as ``paa_project_rows_scaled`` under the new scales.  No host sync, so the step stays one capturable sequence.

Adaptive masking-loss weight: with ``anneal=AnnealConfig(...)`` every clip carries its own alpha_b (alpha0 =
``masking_loss_alpha`` after ``anneal_reset``).  The masking loss runs as ``paa_masking_loss_rows`` with ``alpha_rows``, and
``paa_clip_anneal`` sits where the bound search would: a successful clip whose l_b improves on its best has delta_b, l_b, alpha_b and
the step kept in ``best`` / ``best_loss`` / ``best_alpha`` / ``best_step``; alpha_b rises on success and falls on failure, on the
periods of the config.  ``bound_scale`` (B, device) fixes per-clip bound scales nothing writes (``paa_project_rows_scaled``): the
scales stage 1 of the two-stage run found.

The playback chain: with ``eot_draws=G`` the adversarial example x_b + delta_b of every clip is heard through G
draws of the chain (``chain.ClipChain``: gain, drift, rooms, noise — the links the flags switch on, at least one), R = B * G model
rows, r = b * G + g:

    s_r = a_r (x_b + delta_b)     w_r = noise_r + rooms_r(drift_r(s_r))     loss = sum_r CTC(clamp(w_r, -1, 1), labels_b)
    g_b = sum_g a_r drift_r^T(rooms_r^T(G_r))      then the update and the projections of delta_b against x_b, as above

The model's "clean" operand is a zero buffer and w its p rows, so its clamp is the microphone's clipping.  Launches: [``paa_place_draw``]
-> ``paa_eot_rows`` -> the links -> ``paa_model_fwd_bwd_rows`` on R rows -> the device WER on R rows -> ``paa_eot_vote`` (a clip's
counters are those of its draw that is worst for the attacker) -> ``paa_clip_search`` on the voted counters -> the links' adjoints
-> ``paa_eot_reduce`` -> update -> projections.  Labels and reference rows are given per clip and repeated per draw on the host.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, runtime, synth
from . import chain, place
from .modes import (EOT, FEATURE, LENGTHS, SEARCH_FLAGS, AnnealConfig, Ctx, Modes, SearchConfig, check,  # noqa: F401  (configs: re-exported)
                    replace)
from .pgd import N_STATS, ST_LOSS, PgdStepper, _StepperCore


class ClipStepper(_StepperCore):
    """The per-clip step: ``step(delta, clean, labels)`` updates ``delta`` (B, L) in place, row b from clip b alone."""

    def __init__(self, model, args, length: int, interp=None, spl_thresh=None, optimizer=None, device_wer=False, canon=None,
                 r_cap=None, log_cap=4096, search=None, anneal=None, bound_scale=None, eot_draws=0):
        """``device_wer`` / ``canon`` / ``r_cap`` / ``log_cap`` as PgdStepper's; ``wer_rows[:B]`` keeps the per-clip (errors,
        reference words, hypothesis words) of the last step.  ``search``: a ``SearchConfig`` switches the per-clip bound search on
        (module docstring); it needs ``device_wer=True``, and ``refs`` are then the transcripts success is judged against (the
        target transcript in targeted mode).  Call ``search_reset(B)`` before the first step of every batch.  ``anneal``: an
        ``AnnealConfig`` switches the per-clip alpha schedule on (module docstring); it needs ``device_wer=True`` and
        ``masking_loss_alpha`` > 0 (alpha0), and excludes ``search``.  Call ``anneal_reset(B)`` before the first step of every batch.
        ``bound_scale``: a float32 (B) device tensor of fixed per-clip bound scales for the projections.  ``eot_draws``: G >= 1
        runs every clip through G draws of the playback chain (module docstring); the model then holds B * G rows, so the
        stepper takes at most ``model.max_batch // G`` clips."""
        self.search, self.anneal = search, anneal
        self.G = int(check(Modes.of(args, eot_draws=eot_draws), ("eot_range",)).eot_draws)
        if self.G:       # refusals first: the new rules, then the links' own (masking, eager Adam) in the chain's order
            check(Modes.of(args, eot_draws=self.G), FEATURE + EOT)
            chain.check(args, int(length), int(length))
            if anneal is not None:
                raise NotImplementedError("the alpha schedule needs the masking loss, which does not run through the playback chain")
        if anneal is not None:
            if search is not None:
                raise ValueError("anneal and search cannot share a stepper: the two-stage run uses one stepper per stage")
            m = replace(Modes.of(args), anneal_on=True)
            check(m, ("anneal_alpha0", "anneal_range"), Ctx(anneal=anneal, alpha0=m.alpha))
            if not device_wer:
                raise ValueError("the alpha schedule decides success from the on-device WER counters: build the stepper with "
                                 "device_wer=True")
        if bound_scale is not None and search is not None:
            raise ValueError("bound_scale fixes the scales the bound search would move: pass one or the other")
        if search is not None:
            check(replace(Modes.of(args), search_on=True), SEARCH_FLAGS, Ctx(search=search))
            if not device_wer:
                raise ValueError("the bound search decides success from the on-device WER counters: build the stepper with "
                                 "device_wer=True")
        self.max_batch = int(model.max_batch) // max(self.G, 1)          # clips; the model's rows are clips x draws
        if self.max_batch < 1:
            raise ValueError(f"{self.G} draws per clip need a model of at least that many rows, got max_batch {model.max_batch}")
        super().__init__(model, args, length, interp, spl_thresh, optimizer, device_wer, canon, r_cap, log_cap, self.max_batch,
                         int(length))
        if self.G:
            self.chain = chain.ClipChain(args, self.dev, self.max_batch * self.G, self.L, self.G, place.STREAM_TRAIN)
            self.zero_rows = torch.zeros(self.max_batch * self.G, self.L, dtype=torch.float32, device=self.dev)   # the model's "clean"
            if self.device_wer:
                self.wer_clips = torch.zeros(self.max_batch, 3, dtype=torch.int32, device=self.dev)       # the voted counters
        self.grad_buf = torch.zeros(self.max_batch * self.L, dtype=torch.float32, device=self.dev)
        self.grad = self.grad_buf[: self.L].view(1, self.L)
        self.stats = torch.zeros(N_STATS, dtype=torch.float32, device=self.dev)
        self.mask_rows = torch.zeros(self.max_batch, dtype=torch.float32, device=self.dev)      # l_b of the last step
        if search is not None:
            nb = self.max_batch
            self.scale = torch.ones(nb, dtype=torch.float32, device=self.dev)          # s_b the next projection runs under
            self.best = torch.zeros(nb, self.L, dtype=torch.float32, device=self.dev)  # delta_b of clip b's last success
            self.best_scale = torch.ones(nb, dtype=torch.float32, device=self.dev)     # ... the scale it was projected under
            self.best_step = torch.full((nb,), -1, dtype=torch.int32, device=self.dev)  # ... its step, -1: no success yet
            self.search_step = torch.zeros(1, dtype=torch.int32, device=self.dev)      # device step counter
        if anneal is not None:
            nb = self.max_batch
            self.alpha_rows = torch.full((nb,), self.mask_alpha, dtype=torch.float32, device=self.dev)   # alpha_b of the next step
            self.best = torch.zeros(nb, self.L, dtype=torch.float32, device=self.dev)  # delta_b of clip b's least audible success
            self.best_loss = torch.full((nb,), float("inf"), dtype=torch.float32, device=self.dev)   # ... its l_b
            self.best_alpha = torch.zeros(nb, dtype=torch.float32, device=self.dev)    # ... the alpha it was optimised under
            self.best_step = torch.full((nb,), -1, dtype=torch.int32, device=self.dev)  # ... its step, -1: none kept yet
            self.anneal_step = torch.zeros(1, dtype=torch.int32, device=self.dev)      # device step counter
        self._feat_batch = None          # feature_reset: (B, data_ptr of clean) the reference was computed for
        self.bound_scale = None
        if bound_scale is not None:
            if not (isinstance(bound_scale, torch.Tensor) and bound_scale.is_cuda):
                raise ValueError("bound_scale must be a float32 (B) device tensor: the step reads it on the stream")
            self.bound_scale = _scale_dev(bound_scale, 1, self.dev)

    def feature_reset(self, clean):
        """A new batch under ``--loss_type feature``: the reference of the feature-distance loss, the clean batch's
        last hidden state, is computed here — once per batch, outside any graph: the clips stay the same over a batch's steps —
        into the persistent buffer every later step reads.  Call it before the first step (or ``capture``) of every batch, after
        ``set_lengths``."""
        if not self.modes.feature_on:
            raise RuntimeError("the stepper was built without the feature-distance loss (--loss_type feature)")
        clean = runtime.as_f32_cuda(clean, "clean_audio")
        if clean.dim() != 2 or clean.shape[1] != self.L or clean.shape[0] > self.max_batch:
            raise ValueError(f"clean_audio must be (B <= {self.max_batch}, {self.L}), got {tuple(clean.shape)}")
        self._apply_loss()
        self._feature_reference(clean)
        self._feat_batch = int(clean.shape[0])

    def anneal_reset(self, B=None):
        """A new batch: alpha_rows = alpha0, best_loss = +inf, best_step = -1, step = 0 (stream-ordered fills, outside any graph).
        ``best`` rows and ``best_alpha`` need no reset: they are read only where best_step >= 0."""
        if self.anneal is None:
            raise RuntimeError("the stepper was built without an alpha schedule (anneal=AnnealConfig(...))")
        B = self.max_batch if B is None else int(B)
        self.alpha_rows[:B].fill_(self.mask_alpha)
        self.best_loss[:B].fill_(float("inf"))
        self.best_step[:B].fill_(-1)
        self.anneal_step.zero_()

    def set_masking_alpha(self, alpha: float):
        if getattr(self, "anneal", None) is not None and not float(alpha) > 0:
            raise ValueError("the alpha schedule needs masking_loss_alpha > 0: that value is the weight every clip starts from")
        if getattr(self, "G", 0) and float(alpha) > 0:
            raise NotImplementedError("masking_loss_alpha > 0 does not run through the playback chain (eot_draws): the masking loss "
                                      "pairs the perturbation's frames with the clean clip's frames")
        super().set_masking_alpha(alpha)

    # ---- the playback chain of per-clip perturbations ------------------------------------------------------
    def _site(self, name):
        """The chain's site ``name``; raises when the stepper was built without the chain or with that link off."""
        if not self.G:
            raise RuntimeError("the stepper was built without the playback chain (eot_draws=G)")
        on, off = PgdStepper._SITES[name]
        if not getattr(self.modes, on):
            raise RuntimeError(f"the stepper was built with {off}")
        return getattr(self.chain, name)

    def set_gains(self, gain):
        """Explicit per-row gains (B * G, r = b * G + g) instead of the draw, from the next step on (stream-ordered copy);
        ``set_gains(None)`` returns to drawing.  A captured graph keeps the form it was captured with."""
        pl = self._site("placer")
        pl.set_placement(None if gain is None else [0] * len(gain), gain)

    def set_rooms(self, index):
        """The same for per-row room indices."""
        self._site("reverb").set_rooms(index)

    def set_channel(self, ratio, snr_db=None):
        """The same for per-row clock ratios (and noise SNRs in dB); the noise samples stay fresh."""
        self._site("chan").set_channel(ratio, snr_db)

    def set_eot_step(self, n: int):
        """Device step counters of the chain's next draws (0 at the start of every batch: a clip's draws then depend on the seed,
        its global index, the draw and the step alone)."""
        if not self.G:
            raise RuntimeError("the stepper was built without the playback chain (eot_draws=G)")
        self.chain.set_step(n)

    def set_eot_clip(self, first: int):
        """Global index of the batch's first clip: row r of the following steps draws under the id G * first + r
        (``chain.clip_base``).  A captured graph holds the value it was captured with."""
        if not self.G:
            raise RuntimeError("the stepper was built without the playback chain (eot_draws=G)")
        self.chain.clip_base = self.G * int(first)

    def eval_rows(self, delta, clean, step: int):
        """The B * G rows of evaluation pass ``step``: delta, clean (B, L) through a chain of the evaluation stream
        (place.STREAM_EVAL) whose every counter is set to ``step`` first, at this stepper's ``clip_base`` — so two calls hear the
        same channels and the same noise, whatever ``delta`` holds.  The rows live in the evaluation chain's buffers until the
        next call.  Allocates on first use; for scoring, not for the step."""
        if not self.G:
            raise RuntimeError("the stepper was built without the playback chain (eot_draws=G)")
        delta, clean = self._checked(delta, clean)
        if getattr(self, "_eval_chain", None) is None:
            self._eval_chain = chain.ClipChain(self.args, self.dev, self.max_batch * self.G, self.L, self.G, place.STREAM_EVAL,
                                               with_grad=False)
        ev = self._eval_chain
        ev.clip_base = self.chain.clip_base
        ev.set_step(int(step))
        return ev.rows(delta, clean.shape[0], clean)

    def set_refs(self, refs):
        """As the core's; with the chain on, a batch's (B, r_cap) rows are repeated per draw here on the host."""
        if self.G > 1:
            if refs.dim() != 2 or refs.shape[0] > self.max_batch:
                raise ValueError(f"refs must hold one row per clip (B <= {self.max_batch}), got {tuple(refs.shape)}")
            refs = refs.repeat_interleave(self.G, dim=0)
        super().set_refs(refs)

    def _row_labels(self, labels, B):
        """Labels of B clips -> one row per draw (host-side repeat; rows already B * G are taken as they are)."""
        if self.G > 1 and labels is not None and labels.shape[0] == B:
            labels = labels.repeat_interleave(self.G, dim=0)
        return labels

    def search_reset(self, B=None):
        """A new batch: scale = 1, best_step = -1, step = 0 (stream-ordered fills, outside any graph).  ``best`` rows and
        ``best_scale`` need no reset: they are read only where best_step >= 0."""
        if self.search is None:
            raise RuntimeError("the stepper was built without a bound search (search=SearchConfig(...))")
        B = self.max_batch if B is None else int(B)
        self.scale[:B].fill_(1.0)
        self.best_scale[:B].fill_(1.0)
        self.best_step[:B].fill_(-1)
        self.search_step.zero_()

    def _replay_state(self):
        st = super()._replay_state()
        if self.search is not None:
            st += [self.scale, self.best, self.best_scale, self.best_step, self.search_step]
        if self.anneal is not None:
            st += [self.alpha_rows, self.best, self.best_loss, self.best_alpha, self.best_step, self.anneal_step]
        if self.G:
            st += self.chain.counters()
        return st

    def _check_adam_shape(self):
        if self.adam_p.dim() != 2 or self.adam_p.shape[1] != self.L or self.adam_p.shape[0] > self.max_batch:
            raise ValueError(f"optimizer parameter has shape {tuple(self.adam_p.shape)}, expected (B, {self.L}) with "
                             f"B <= {self.max_batch}")

    def _checked(self, delta, clean):
        delta = runtime.as_f32_cuda(delta, "delta")
        clean = runtime.as_f32_cuda(clean, "clean_audio")
        if clean.dim() != 2 or clean.shape[1] != self.L:
            raise ValueError(f"clean_audio must be (B, {self.L}), got {tuple(clean.shape)}")
        if tuple(delta.shape) != tuple(clean.shape):
            raise ValueError(f"per-clip perturbation must be (B, L) = {tuple(clean.shape)}, got {tuple(delta.shape)}")
        if clean.shape[0] > self.max_batch:
            raise ValueError(f"batch {clean.shape[0]} exceeds the model's max_batch {self.max_batch}")
        return delta, clean

    def _body(self, delta, clean, labels, want_logits=True, logits_out=None):
        lib, L, B = _lib.lib(), self.L, clean.shape[0]
        if self.modes.feature_on and self._feat_batch != B:
            raise RuntimeError("--loss_type feature: call feature_reset(clean) before the first step of every batch "
                               f"(the reference holds {self._feat_batch} clips, the batch {B})")
        grad = self.grad_buf[: B * L].view(B, L)
        self.grad = grad
        G = self.G
        R = B * G if G else B                      # rows the model sees
        out = {"grad": self.chain.placer.grad_rows[:R] if G else grad, "stats": self.stats}
        if logits_out is not None:
            out["logits"] = logits_out
        if G:       # the model's "clean" operand is zero and its p rows are what the microphone hears: its clamp is the clipping
            r = self.model.fwd_bwd(self.zero_rows[:R], self.chain.rows(delta, B, clean), labels, self.direction, want_grad=True,
                                   want_logits=want_logits, out=out)
            r["grad_rows"] = r["grad"]
        else:
            r = self.model.fwd_bwd(clean, delta, labels, self.direction, want_grad=True, want_logits=want_logits, out=out)
        ac = self.anneal
        if self.mask_alpha > 0:
            self._masking_loss(delta, clean, grad, self.mask_rows[:B], None if ac is None else self.alpha_rows)
            r["masking_loss"] = self.mask_rows[:B]
        counts = None
        if self.device_wer:
            self._wer(r["logits"], R)
            counts = self.wer_rows
            if G:       # a clip's counters are those of its draw that is worst for the attacker: success means every draw succeeded
                counts = self.wer_clips
                with torch.cuda.device(self.dev):
                    _lib.check(lib.paa_eot_vote(_lib.ptr(self.wer_rows), B, G, int(self.direction < 0), _lib.ptr(counts),
                                                _lib.stream_ptr()))
        with torch.cuda.device(self.dev):
            st = _lib.stream_ptr()
            sc = self.search
            if sc is not None:       # the counters are those of the delta that entered the step: keep it BEFORE the update
                _lib.check(lib.paa_clip_search(_lib.ptr(delta), B, L, _lib.ptr(counts), int(bool(sc.targeted)),
                                               int(sc.wer_milli), float(sc.shrink), float(sc.floor_scale), _lib.ptr(self.scale),
                                               _lib.ptr(self.best), _lib.ptr(self.best_scale), _lib.ptr(self.best_step),
                                               _lib.ptr(self.search_step), st))
            if ac is not None:       # ... and so is l_b: the delta kept is the delta judged
                _lib.check(lib.paa_clip_anneal(_lib.ptr(delta), B, L, _lib.ptr(self.wer_rows), _lib.ptr(self.mask_rows),
                                               int(bool(ac.targeted)), int(ac.wer_milli), int(ac.up_every), int(ac.down_every),
                                               float(ac.up), float(ac.down), float(ac.alpha_min), float(ac.alpha_max),
                                               _lib.ptr(self.alpha_rows), _lib.ptr(self.best), _lib.ptr(self.best_loss),
                                               _lib.ptr(self.best_alpha), _lib.ptr(self.best_step), _lib.ptr(self.anneal_step), st))
            if G:       # the chain's adjoints, then the sum over every clip's draws into its own row
                self.chain.reduce(B, grad)
            self._update(delta, grad, B * L)
            scale = self.scale if sc is not None else self.bound_scale
            if scale is not None and scale.numel() < B:
                raise ValueError(f"bound_scale holds {scale.numel()} values, the batch has {B} clips")
            for prm in self._prm:
                if scale is not None:
                    _lib.check(lib.paa_project_rows_scaled(self.proj.h, prm, _lib.ptr(delta), _lib.ptr(delta), B, _lib.ptr(clean),
                                                           L, _lib.ptr(scale), st))
                else:
                    _lib.check(lib.paa_project_rows(self.proj.h, prm, _lib.ptr(delta), _lib.ptr(delta), B, _lib.ptr(clean), L, st))
                if self.lengths_on:
                    _lib.check(lib.paa_mask_tail_rows(_lib.ptr(delta), B, L, _lib.ptr(self.model._lengths), st))
        if self.device_wer:
            self.stats_log.push(self.stats)
        r["loss"] = self.stats[ST_LOSS]
        r["grad"] = grad
        return r

    def step(self, delta: torch.Tensor, clean: torch.Tensor, labels: torch.Tensor, want_logits=True, logits_out=None,
             refs=None, lengths=None):
        """In place on ``delta`` (B, L).  Returns dict(loss: 0-d device tensor, the sum over the clips, logits, grad (B, L)).
        ``refs`` / ``lengths`` as PgdStepper.step."""
        if refs is not None:
            self.set_refs(refs)
        if lengths is not None:
            self.set_lengths(lengths)
        delta, clean = self._checked(delta, clean)
        self._check_p(delta)
        self._pre_step()
        return self._body(delta, clean, self._row_labels(labels, clean.shape[0]), want_logits, logits_out)

    def capture(self, delta, clean, labels, logits_out=None, refs=None, lengths=None):
        """One step on fixed buffers as ONE hipGraph (``refs`` / ``lengths`` as PgdStepper.capture).  Returns (graph, result dict);
        ``graph.replay()`` re-runs the step in place on ``delta`` with whatever ``clean`` / ``labels`` hold.  With Adam the graph is
        wrapped so that every replay first pushes the step's scalars, and the warm-up step is undone (delta, moments and step
        count as before the call).  With a bound search the warm-up step is undone with either update — delta and the search
        buffers (scale, best, best_scale, best_step, step) are as before the call, so the first replay is the step an eager
        call would have been.  The same holds for the alpha schedule and its buffers (alpha_rows, best, best_loss, best_alpha,
        best_step, step), and for the playback chain (``eot_draws``): delta and every draw counter are as before the call, so
        capture plus n replays is n eager steps, draw for draw."""
        delta, clean = self._checked(delta, clean)
        keep = delta.detach().clone() if self.search is not None or self.anneal is not None or self.G else None
        if self.G and logits_out is None:          # one row of logits per draw
            logits_out = torch.empty(clean.shape[0] * self.G, self.model.frames, self.model.arch.vocab_size, device=self.dev)
        lab, logits_out = self._warm_up(delta, clean, self._row_labels(labels, clean.shape[0]), logits_out, refs, lengths)
        if keep is not None:
            delta.detach().copy_(keep)
        return self._capture_body(delta, clean, lab, logits_out)


# ---------------------------------------------------------------------------------------------------- host helpers
def init_rows(length: int, indices, seed: int = 5) -> np.ndarray:
    """(len(indices), L) float32 standard normals: the stand-in of build.init_perturbation's ``torch.randn(1, L)`` for each
    clip, keyed by the clip's GLOBAL index (its position in the split), so that a clip's draw depends neither on the batch it
    lands in nor on the number of ranks."""
    out = np.empty((len(indices), int(length)), dtype=np.float32)
    for r, i in enumerate(indices):
        out[r] = synth.normal(synth.key_of(f"p0_clip{int(i)}", int(seed)), int(length)).astype(np.float32)
    return out


def _lengths_dev(lengths, B, L, dev):
    """Host-validated per-clip sample counts ([1, L], one per clip) as an int32 device tensor."""
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda and lengths.dtype == torch.int32 and lengths.numel() >= B:
        return lengths[:B].contiguous()
    t = torch.as_tensor(lengths).detach().cpu()
    if t.dim() != 1 or t.numel() != B or t.is_floating_point():
        raise ValueError(f"lengths must hold {B} integers, got shape {tuple(t.shape)} dtype {t.dtype}")
    if int(t.min()) < 1 or int(t.max()) > L:
        raise ValueError(f"clip lengths must lie in [1, {L}], got [{int(t.min())}, {int(t.max())}]")
    return t.to(torch.int32).to(dev)


def mask_tail_rows(delta: torch.Tensor, lengths) -> torch.Tensor:
    """delta_b[len_b:] = 0 for every row, in place (paa_mask_tail_rows)."""
    B, L = delta.shape
    ln = _lengths_dev(lengths, B, L, delta.device)
    with torch.cuda.device(delta.device):
        _lib.check(_lib.lib().paa_mask_tail_rows(_lib.ptr(delta), B, L, _lib.ptr(ln), _lib.stream_ptr()))
    return delta


def _scale_dev(scale, B, dev):
    """The per-row bound scales as a float32 (B) device tensor.  A host array is validated (finite, > 0); a device tensor is
    taken as it is: the kernels treat a value that is not a finite positive number as 1."""
    if isinstance(scale, torch.Tensor) and scale.is_cuda:
        if scale.dtype != torch.float32 or scale.dim() != 1 or scale.numel() < B or not scale.is_contiguous():
            raise ValueError(f"scale must be a contiguous float32 tensor of at least {B} elements, got {scale.dtype} "
                             f"{tuple(scale.shape)}")
        return scale.to(dev)
    s = np.asarray(scale.cpu() if isinstance(scale, torch.Tensor) else scale, dtype=np.float64).reshape(-1)
    if s.size != B:
        raise ValueError(f"scale must hold one value per row ({B}), got {s.size}")
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError(f"every bound scale must be finite and > 0, got {s.tolist()}")
    return torch.from_numpy(s.astype(np.float32)).to(dev)


def project_rows(delta: torch.Tensor, clean: torch.Tensor, args, interp=None, spl_thresh=None, lengths=None, scale=None) -> torch.Tensor:
    """perturbation_constraint (train.py:69-99) on every row of ``delta`` (B, L) against its own clip of ``clean`` (B, L),
    in place; the norms of ``args.norm_type`` in order.  ``lengths``: delta_b[len_b:] is re-zeroed after every projection.
    ``scale`` (B): row b's bound is tightened by scale[b] (paa_project_rows_scaled)."""
    m = Modes.of(args)
    if lengths is not None:
        check(replace(m, lengths_on=True), LENGTHS)
    delta = runtime.as_f32_cuda(delta, "delta")
    clean = runtime.as_f32_cuda(clean, "clean_audio")
    if delta.dim() != 2 or tuple(delta.shape) != tuple(clean.shape):
        raise ValueError(f"delta {tuple(delta.shape)} and clean_audio {tuple(clean.shape)} must both be (B, L)")
    B, L = delta.shape
    pr = runtime.get_proj(args, delta.device, B, L, interp)
    sc = None if scale is None else _scale_dev(scale, B, delta.device)
    with torch.cuda.device(delta.device):
        for n in m.norms:
            if n not in _lib.NORM_IDS:
                raise ValueError(f"Unknown norm_type: {n!r}")
            if n == "max_phon":
                pr.set_spl_thresh(spl_thresh)
            if sc is None:
                _lib.check(_lib.lib().paa_project_rows(pr.h, runtime.params_of(args, n), _lib.ptr(delta), _lib.ptr(delta), B,
                                                       _lib.ptr(clean), L, _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().paa_project_rows_scaled(pr.h, runtime.params_of(args, n), _lib.ptr(delta), _lib.ptr(delta), B,
                                                              _lib.ptr(clean), L, _lib.ptr(sc), _lib.stream_ptr()))
            if lengths is not None:
                mask_tail_rows(delta, lengths)
    return delta


def compose_rows(clean: torch.Tensor, delta: torch.Tensor, lengths=None) -> torch.Tensor:
    """clamp(clean_b + delta_b, -1, 1) for every clip (the adversarial waveforms the entry point writes); with ``lengths``,
    exactly 0 for the samples i >= len_b (attack the utterance, then pad)."""
    clean = runtime.as_f32_cuda(clean, "clean_audio")
    delta = runtime.as_f32_cuda(delta, "delta")
    B, L = clean.shape
    out = torch.empty_like(clean)
    with torch.cuda.device(clean.device):
        _lib.check(_lib.lib().paa_compose_clamp_rows(_lib.ptr(clean), _lib.ptr(delta), delta.shape[0] if delta.dim() == 2 else 1,
                                                     _lib.ptr(out), B, L, _lib.stream_ptr()))
    if lengths is not None:
        mask_tail_rows(out, lengths)
    return out


def clip_nll(model, logits: torch.Tensor, labels: torch.Tensor, frames=None) -> torch.Tensor:
    """Per-clip CTC loss (B,) of logits (B, T, V) on the device (paa_ctc, HF reduction 'sum' per clip); ``frames`` (B) int32 on
    the device (``model.frame_counts``): clip b aligns over its first frames[b] frames (paa_ctc_len)."""
    lab = labels.to(device=logits.device, dtype=torch.int32).contiguous()
    B, T, V = logits.shape
    S = lab.shape[1]
    L = _lib.lib()
    work = torch.empty(int(L.paa_ctc_work_floats(B, T, V, S)), dtype=torch.float32, device=logits.device)
    nll = torch.empty(B, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        if frames is None:
            _lib.check(L.paa_ctc(_lib.ptr(logits.contiguous()), _lib.ptr(lab), B, T, V, S, int(model.arch.pad_token_id), 1.0,
                                 _lib.ptr(nll), None, _lib.ptr(work), _lib.stream_ptr()))
        else:
            if frames.dtype != torch.int32 or frames.device != logits.device or frames.numel() < B:
                raise ValueError(f"frames must be int32 ({B},) on the device of the logits")
            _lib.check(L.paa_ctc_len(_lib.ptr(logits.contiguous()), _lib.ptr(lab), _lib.ptr(frames), B, T, V, S,
                                     int(model.arch.pad_token_id), 1.0, _lib.ptr(nll), None, _lib.ptr(work), _lib.stream_ptr()))
    return nll
