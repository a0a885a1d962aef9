"""The PGD inner step as one launch sequence on the device (SURVEY §8a S1-S6 + P0).  ``_StepperCore`` holds what the universal step
(``PgdStepper``, here) and the per-clip step (``clip_attack.ClipStepper``) share; a mode adds launches to the plain sequence:

    mode (switched on by)                      launches                                                  where
    -----------------------------------------  --------------------------------------------------------  --------------------------------
    plain universal step                       paa_model_fwd_bwd, paa_sign_step, paa_project per norm     (forward + CTC + backward to the
                                                                                                          waveform, update, projections)
    per-clip step (ClipStepper)                paa_model_fwd_bwd_rows, paa_sign_step over B*L,            the whole sequence; no collective
                                               paa_project_rows per norm
    Adam (``optimizer=``)                      paa_adam_step                                              in place of paa_sign_step
    masking loss (``masking_loss_alpha`` > 0)  paa_masking_loss                                           right after the backward pass
    device WER (``device_wer=True``)           paa_argmax_ids, paa_wer_counts                             after the masking loss
                                               paa_stats_push                                             after the last projection
    collective (several ranks, or              paa_batch_stats (snr / tv only)                            last before the all-reduce
    ``force_collective``; universal only)      all_reduce(packed, SUM)                                    between backward and update
                                               paa_project_ext                                            in place of paa_project (snr / tv)
    placement (``perturbation_seconds`` /      paa_place_draw (not after ``set_placement``),              before the forward pass
    ``place_shift`` / ``place_gain_db``;       paa_place_rows
    universal only)                            paa_model_fwd_bwd_rows                                     in place of paa_model_fwd_bwd
                                               paa_place_reduce                                           right after the backward pass
    room responses (``rir_bank``; universal    paa_rir_draw (not after ``set_rooms``), paa_rir_apply      between paa_place_rows and the forward
    only; runs the placement launches too,     paa_rir_apply (adjoint)                                    between the backward pass and
    at shift 0 / gain 1 when placement is off)                                                            paa_place_reduce
    playback channel (``drift_ppm`` /          paa_chan_draw (not after ``set_channel``),                 between paa_place_rows and the rooms
    ``noise_snr_db``; universal only; runs     paa_drift_apply (drift only)
    the placement launches too, likewise)      paa_noise_add (noise only: two launches)                   last before the forward pass
                                               paa_drift_apply (adjoint; drift only)                      right before paa_place_reduce

    margin loss (``loss_type`` = "margin",     inside paa_model_fwd_bwd{,_rows}: the alignment-margin      DESIGN.md §6l
    targeted only)                             sequence (paa_align_margin) in place of CTC; slot 0 of the
                                               stats then holds the margin loss
    feature loss (``loss_type`` = "feature",   paa_model_features(clean) into the stepper's reference      DESIGN.md §6q
    untargeted only)                           buffer: before paa_model_fwd_bwd in every universal step,
                                               once per batch (``feature_reset``) for the per-clip step;
                                               inside paa_model_fwd_bwd{,_rows}: paa_feature_cos in place
                                               of the loss sequence, no lm_head input-gradient product;
                                               slot 0 of the stats then holds the feature distance
    true clip lengths (``lengths=`` /          inside paa_model_fwd_bwd{,_rows}: frame counts, zeroed      DESIGN.md §6h
    ``set_lengths``)                           frames, masked compose / attention / CTC
                                               paa_model_frame_counts, paa_argmax_ids_len                 in place of paa_argmax_ids (device WER)
                                               paa_mask_tail_rows (per-clip step only)                    after every paa_project_rows
    bound search (``search=SearchConfig``;     paa_clip_search                                           after the device WER counters, before
    per-clip step only; needs device WER)                                                                 the update
                                               paa_project_rows_scaled                                    in place of paa_project_rows
    alpha schedule (``anneal=AnnealConfig``;   paa_masking_loss_rows                                      in place of paa_masking_loss
    per-clip step only; needs device WER and   paa_clip_anneal                                            after the device WER counters, before
    ``masking_loss_alpha`` > 0; no search)                                                                the update
    fixed bound scales (``bound_scale=``)      paa_project_rows_scaled                                    in place of paa_project_rows
    playback chain of per-clip steps           paa_eot_rows, then the links' launches above on B * G       before the forward pass, in place of
    (``eot_draws=G``; per-clip step only;      rows (paa_place_draw for the gains only)                    paa_place_rows
    at least one link on)                      paa_eot_vote (device WER only)                              after the device WER counters
                                               the links' adjoints, paa_eot_reduce                         right before the update

A mode that is off adds no launch: alpha = 0, ``device_wer=False``, placement off, room responses off, the channel off, lengths off,
no bound search and no alpha schedule are the plain step, bit for bit.

Which modes may run together, and which refusal wins when several apply, is decided in one table: training_utils/modes.py.  What
a mode means is written where it is built: place.py, rir.py (§6g), channel.py (§6k) and chain.py, which orders the
three (``chain.PlaybackChain``), ``set_lengths`` and PaaModel.set_lengths (§6h).

The packed vector is ``[ grad (Lp) | loss, sum clean^2, TV(clean), wer_errors, wer_ref_words, clips, masking loss, 0 ]`` in
float32; the 8 stat slots are defined HERE (ST_*) and documented in include/paa_hip.h (paa_model_fwd_bwd, d_stats).  Every rank
holds the full universal perturbation and a shard of the utterances; HF's CTC reduction is 'sum', so the global gradient is the sum
of the shard gradients and ONE all-reduce of the packed vector per step (RCCL over xGMI via torch.distributed's "nccl" backend)
suffices: every rank then applies the identical update and projection, and the replicas stay bit-identical without a broadcast.
Slots 1, 2 and 5 are there because project_snr / project_tv use whole-GLOBAL-batch statistics (projections.py:11-35, 56-66) and
the SNR target norm the global ``clean.numel()``: ``paa_batch_stats`` writes this rank's sums and clip count, the all-reduce adds
them (the count is a small integer, exact in f32) and ``paa_project_ext`` reads the sums on the device, so ranks may hold different
numbers of clips, in any step.  Slots 3 and 4 carry the word errors / reference words: of the PREVIOUS step, counted on the host
(``set_wer_counts``), or of THIS step with ``device_wer``, which also appends the global stats to a device log
(``read_log``: ONE readback per epoch).  Slot 6 is sum_b l_b of the masking loss, whose gradient ``paa_masking_loss``
subtracts BEFORE the all-reduce.  Host -> device scalars of a step (the host's WER counters, Adam's step scalars, alpha) travel
through a ring of pinned slots (``_HostRing``) by asynchronous copies, so captured graphs follow them on replay.
"""
from __future__ import annotations

import contextlib

import torch

from .. import _lib, runtime
from . import chain, channel, modes, place, rir
from .build import batch_lengths, unpack_batch  # noqa: F401  (re-exported)
from .modes import Ctx, Modes, replace

FREQ_NORMS = ("fletcher_munson", "min_max_freqs", "max_phon")
N_STATS = 8
ST_LOSS, ST_SQ, ST_TV, ST_WER_ERR, ST_WER_REF, ST_CLIPS, ST_MASK_LOSS = 0, 1, 2, 3, 4, 5, 6
RING = 4


def adam_unsupported(optimizer):
    """None if ``optimizer`` is the plain torch.optim.Adam the device step implements (one param group holding one tensor,
    float hyper-parameters, weight_decay 0, amsgrad / maximize / capturable / differentiable / fused off, the foreach
    kernels), else the name of the first option it does not cover."""
    if type(optimizer) is not torch.optim.Adam:
        return f"optimizer {type(optimizer).__name__}"
    if len(optimizer.param_groups) != 1 or len(optimizer.param_groups[0]["params"]) != 1:
        return "more than one parameter"
    g = optimizer.param_groups[0]
    if g.get("weight_decay", 0) != 0:
        return "weight_decay"
    for k in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
        if g.get(k):
            return k
    if g.get("foreach") is False:
        return "foreach=False"
    if any(isinstance(x, torch.Tensor) for x in (g["lr"], *g["betas"], g["eps"])):
        return "tensor hyper-parameters"
    return None


def lengths_refusal(args):
    """None, or why ``args`` cannot run with true clip lengths (``--clip_lengths true``), whether or not the flag is set."""
    m = Modes.of(args, clip_lengths="true")
    return next((modes.RULES[k].msg for k in modes.LENGTHS if modes.RULES[k].when(m, Ctx())), None)


def check_clip_lengths(args):
    """Refusals of ``--clip_lengths true``, raised before any launch or collective; True when the mode is on."""
    return modes.check(Modes.of(args), modes.LENGTHS).lengths_on


def masking_route(norm_type, world: int) -> None:
    """The masking norm bounds the universal perturbation by the minimum of every clip's bound: with several ranks that is a
    MIN over the ranks' shards, which the step's one SUM all-reduce does not carry.  Raises NotImplementedError (on every
    rank, before any collective) for a data-parallel masking run; one rank, force_collective included, is fine."""
    modes.check(Modes.of(norm_type=norm_type), ("route",), Ctx(world))


class StatsLog:
    """Device log of per-step stats rows: ``push`` is one launch (``paa_stats_push``: row ``cursor % cap`` <- stats, cursor += 1
    on the device; allocation-free, capturable), ``read`` the one synchronising readback — the rows since the last read, oldest
    first, as a CPU float32 (n, N_STATS) tensor."""

    def __init__(self, dev, cap: int = 4096, n: int = N_STATS):
        self.dev, self.cap, self.n = dev, int(cap), int(n)
        self.log = torch.zeros(self.cap, self.n, dtype=torch.float32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)

    def push(self, stats):
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_stats_push(_lib.ptr(stats), self.n, _lib.ptr(self.log), _lib.ptr(self.cursor), self.cap,
                                                 _lib.stream_ptr()))

    def read(self, reset: bool = True):
        n = int(self.cursor.item())
        if n > self.cap:
            raise RuntimeError(f"stats log overflow: {n} rows pushed into {self.cap} since the last read")
        rows = self.log[:n].cpu()
        if reset:
            self.cursor.zero_()
        return rows


def adam_scalars(lr, beta1, beta2, step):
    """[-lr / (1 - beta1^t), sqrt(1 - beta2^t)] in double, as torch/optim/adam.py _multi_tensor_adam (capturable=False)
    computes step_size and bias_correction2_sqrt; the foreach kernels round them to f32."""
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return (lr / bc1) * -1, bc2 ** 0.5


class _HostRing:
    """RING pinned slots of ``n`` floats for the host -> device scalars of a step.  The copies out of a slot are asynchronous, so
    the slot is rewritten only after the event behind its copies has completed."""

    def __init__(self, n: int, dev):
        self.dev = dev
        self.slots = [torch.zeros(n, dtype=torch.float32).pin_memory() for _ in range(RING)]
        self.events = [None] * RING
        self.i = 0

    @contextlib.contextmanager
    def slot(self):
        """``with ring.slot() as h``: the next slot, free to write; the block fills it and issues its ``copy_(h[...],
        non_blocking=True)`` on the current stream, whose position is recorded behind them."""
        k = self.i % RING
        self.i += 1
        if self.events[k] is not None:
            self.events[k].synchronize()
        yield self.slots[k]
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self.events[k] = ev


class _StepperCore:
    """What the universal and the per-clip step share: the norms and their params, the projection context, the adopted Adam, the
    host scalars of a step, the masking-loss term, the device WER counters with the stats log, the update launch and the
    warm-up of ``capture()``.  A leaf allocates ``grad`` / ``stats``, checks its shapes, and orders the launches in ``_body``."""
    collective = False                  # PgdStepper alone runs the packed all-reduce ...
    _wer_next = (0.0, 0.0)              # ... and carries the host's WER counters behind its gradient

    def __init__(self, model, args, length, interp, spl_thresh, optimizer, device_wer, canon, r_cap, log_cap, proj_rows, proj_len):
        self.model, self.args, self.L = model, args, int(length)
        self.dev = model.device
        self.modes = modes.check(Modes.of(args), modes.MARGIN + modes.FEATURE)
        self.norms = list(self.modes.norms)
        for n in self.norms:
            if n not in _lib.NORM_IDS:
                raise ValueError(f"Unknown norm_type: {n!r}")                  # train.py:98
        self.direction = +1 if args.attack_mode == "untargeted" else -1          # train.py:124
        self._prm = [runtime.params_of(args, n) for n in self.norms]
        self.proj = runtime.get_proj(args, self.dev, proj_rows, proj_len, interp)
        if spl_thresh is not None:
            self.proj.set_spl_thresh(spl_thresh)
        self.optimizer = optimizer
        if optimizer is not None:
            why = adam_unsupported(optimizer)
            if why is not None:
                raise NotImplementedError(f"the device Adam step does not implement {why}")
            self.adam_p = optimizer.param_groups[0]["params"][0]
            self._check_adam_shape()
            self.adam_scal = torch.zeros(2, dtype=torch.float32, device=self.dev)
            self.adam_grad = torch.zeros_like(self.adam_p, dtype=torch.float32, device=self.dev)
        # one slot per step: [wer errors, wer reference words, adam step_size, adam bias_correction2_sqrt]
        self._ring = _HostRing(4, self.dev) if (self.collective or optimizer is not None) else None
        self._init_masking_loss()
        self._init_device_wer(device_wer, canon, r_cap, log_cap)
        # the feature-distance loss: the persistent reference buffer the model reads on the stream
        self.feat_ref = None
        if self.modes.feature_on:
            self.feat_ref = torch.zeros(int(model.max_batch), int(model.frames), int(model.arch.hidden_size), dtype=torch.float32,
                                        device=self.dev)
        self._apply_loss()
        self._lengths_captured = None        # capture() records whether the captured launch sequence runs in the length mode

    # ---- the loss of the step -------------------------------------------------------------------------
    def _apply_loss(self):
        """``--loss_type`` / ``--margin_kappa`` of ``args`` go to the model (``PaaModel.set_loss``; a host-side switch read by every
        later ``fwd_bwd``).  Steppers of different loss types may share a model: every eager step sets its own; a captured graph
        keeps the launches it was captured with.  A model that never saw the margin loss is not touched.  ``--loss_type feature``
         hands the model this stepper's reference buffer (``PaaModel.set_feature_loss``); the two losses exclude
        each other on the model, so the one that is going off is switched off first."""
        kind = 1 if self.modes.margin_on else 0
        kappa = float(self.modes.kappa) if kind else 0.0
        ref = self.feat_ref if self.modes.feature_on else None
        if ref is None and getattr(self.model, "feature_ref", None) is not None:
            self.model.set_feature_loss(None)
        if (getattr(self.model, "loss_kind", 0), getattr(self.model, "loss_kappa", 0.0)) != (kind, kappa):
            self.model.set_loss(kind, kappa)
        if ref is not None and getattr(self.model, "feature_ref", None) is not ref:
            self.model.set_feature_loss(ref)

    def _feature_reference(self, clean):
        """The reference of the feature-distance loss: the clean batch's last hidden state into rows [0, B) of the persistent
        buffer (``paa_model_features``: the forward pass up to the final LayerNorm and one copy; capturable once the model's f32
        hidden buffer exists, which ``_apply_loss`` saw to).  Under true clip lengths the rows t >= T_b are zeros and not read."""
        self.model.features(clean, None, out=self.feat_ref)

    # ---- true clip lengths ------------------------------------------------------------------------------------------
    @property
    def lengths_on(self):
        return bool(self.model.lengths_on)

    def set_lengths(self, lengths):
        """Per-clip sample counts from the next step on (host-validated, copied into the model's persistent buffer; a captured
        graph follows it), or None to switch the mode off.  Refused for the modes the table's "lengths" entry names, and — like
        the masking loss — the mode cannot be switched on or off after ``capture()``."""
        on = lengths is not None
        if on:
            m = modes.check(replace(self.modes, lengths_on=True), modes.LENGTHS)
            modes.check(replace(m, alpha=self.mask_alpha), modes.LENGTHS)          # an alpha set after construction
        if self._lengths_captured is not None and on != self._lengths_captured:
            raise ValueError("clip lengths cannot be switched on or off after capture(): the captured launch sequence "
                             f"{'runs' if self._lengths_captured else 'does not run'} in the length mode; capture the step again")
        with torch.cuda.device(self.dev):
            return self.model.set_lengths(lengths)

    def _frames(self, B):
        """T_b of the model's current length buffer in a fixed int32 buffer (one launch, capturable); None with lengths off."""
        if not self.lengths_on:
            return None
        if getattr(self, "frames_buf", None) is None:
            self.frames_buf = torch.ones(int(self.model.max_batch), dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().paa_model_frame_counts(self.model.h, int(B), _lib.ptr(self.frames_buf), _lib.stream_ptr()))
        return self.frames_buf

    # ---- on-device WER counters and the stats log ----------------------------------------------------------------
    def _init_device_wer(self, device_wer, canon=None, r_cap=None, log_cap=4096):
        self.device_wer = bool(device_wer)
        if not self.device_wer:
            return
        from ..core import loss_helpers
        canon = loss_helpers.canon_table(None) if canon is None else canon
        self.canon = canon.to(self.dev, torch.int32).contiguous()
        self.r_cap = int(loss_helpers.R_CAP if r_cap is None else r_cap)
        nb = int(self.model.max_batch)
        self.refs = torch.full((nb, self.r_cap), -1, dtype=torch.int32, device=self.dev)
        self.ids = torch.zeros(nb * int(self.model.frames), dtype=torch.int16, device=self.dev)
        self.wer_rows = torch.zeros(nb, 3, dtype=torch.int32, device=self.dev)     # (errors, ref words, hyp words) per clip
        self.wer_batch = 0                                                         # clips of the last step
        self.stats_log = StatsLog(self.dev, log_cap, N_STATS)

    def set_refs(self, refs):
        """Stream-ordered copy of the batch's reference rows (``loss_helpers.encode_refs``: (B, r_cap) int32, pinned or on the
        device) into the fixed buffer the step — eager or captured — reads; call it before ``step`` / ``replay``."""
        if not self.device_wer:
            raise RuntimeError("set_refs needs a stepper built with device_wer=True")
        if refs.dtype != torch.int32 or refs.dim() != 2 or refs.shape[1] != self.r_cap or refs.shape[0] > self.refs.shape[0]:
            raise ValueError(f"refs must be int32 (B <= {self.refs.shape[0]}, {self.r_cap}), got {refs.dtype} {tuple(refs.shape)}")
        self.refs[: refs.shape[0]].copy_(refs, non_blocking=True)

    def _wer(self, logits, B):
        """paa_argmax_ids + paa_wer_counts on the step's logits: per-clip counters -> wer_rows[:B], their sums -> slots 3, 4."""
        if logits is None:
            raise ValueError("device_wer needs the step's logits (want_logits=True)")
        from ..core import loss_helpers
        self.wer_batch = B
        loss_helpers.wer_counts_device(logits, self.refs[:B], self.canon, out=self.wer_rows[:B],
                                       sums=self.stats[ST_WER_ERR:ST_WER_REF + 1], ids_out=self.ids[: B * logits.shape[1]],
                                       frames=self._frames(B), blank=int(self.model.arch.pad_token_id))

    def read_log(self):
        """The stats rows of the steps since the last call, oldest first: CPU float32 (n, N_STATS), global sums after the
        collective (slot 0 CTC loss, 3 / 4 word errors / reference words, 6 masking loss).  The one host sync of an epoch."""
        return self.stats_log.read()

    # ---- masking-threshold loss term ---------------------------------------------------------------------------
    def _init_masking_loss(self):
        self.mask_alpha = 0.0
        self.alpha_dev = None
        self._alpha_captured = None          # capture() records whether the captured launch sequence holds the term
        self._mask_prm = runtime.params_of(self.args, "masking")          # paa_masking_loss reads masking_margin_db only
        if self.modes.alpha != 0:
            self.set_masking_alpha(self.modes.alpha)

    def set_masking_alpha(self, alpha: float):
        """Weight of the masking-threshold loss term from the next step on.  The value goes to a one-float device tensor by a
        stream-ordered copy from pinned memory, so eager steps and captured graphs alike follow it without recapture.  Whether
        the term is in the launch sequence at all (alpha > 0) is fixed by ``capture()``: switching it on or off afterwards
        raises."""
        alpha = float(alpha)
        lengths_on = bool(getattr(getattr(self, "model", None), "lengths_on", False))
        modes.check(replace(getattr(self, "modes", None) or Modes.of(), alpha=alpha, lengths_on=lengths_on), ("alpha_range", "len_alpha"))
        if self._alpha_captured is not None and (alpha > 0) != self._alpha_captured:
            raise ValueError("masking_loss_alpha cannot switch between 0 and > 0 after capture(): the captured launch sequence "
                             f"{'holds' if self._alpha_captured else 'does not hold'} the loss term; capture the step again")
        if alpha > 0:
            if self.alpha_dev is None:
                self.alpha_dev = torch.zeros(1, dtype=torch.float32, device=self.dev)
                self._alpha_ring = _HostRing(1, self.dev)
            with torch.cuda.device(self.dev), self._alpha_ring.slot() as h:
                h[0] = alpha
                self.alpha_dev.copy_(h, non_blocking=True)
        elif self.mask_alpha > 0:
            self.stats[ST_MASK_LOSS] = 0.0
        self.mask_alpha = alpha

    def _masking_loss(self, p, clean, grad, loss_rows=None, alpha_rows=None):
        """grad -= alpha * grad(sum_b l_b); sum_b l_b -> slot 6.  p (rows, L), rows in {1, B}.  ``alpha_rows`` (B) on the device: row
        b's own weight through paa_masking_loss_rows; None is paa_masking_loss with the stepper's scalar."""
        B = clean.shape[0]
        with torch.cuda.device(self.dev):
            if alpha_rows is not None:
                _lib.check(_lib.lib().paa_masking_loss_rows(self.proj.h, self._mask_prm, _lib.ptr(p), p.shape[0], _lib.ptr(clean), B,
                                                            self.L, _lib.ptr(alpha_rows), B, _lib.ptr(grad), _lib.ptr(loss_rows),
                                                            _lib.ptr(self.stats[ST_MASK_LOSS:ST_MASK_LOSS + 1]), None,
                                                            _lib.stream_ptr()))
                return
            _lib.check(_lib.lib().paa_masking_loss(self.proj.h, self._mask_prm, _lib.ptr(p), p.shape[0] if p.dim() == 2 else 1,
                                                   _lib.ptr(clean), B, self.L, _lib.ptr(self.alpha_dev), _lib.ptr(grad),
                                                   _lib.ptr(loss_rows), _lib.ptr(self.stats[ST_MASK_LOSS:ST_MASK_LOSS + 1]), None,
                                                   _lib.stream_ptr()))

    # ---- the update -------------------------------------------------------------------------------------------------
    def adam_consts(self):
        """(w1, beta2, omb2, eps) of the optimizer's param group as the foreach kernels see them (f32 by value)."""
        g = self.optimizer.param_groups[0]
        b1, b2 = g["betas"]
        return float(1 - b1), float(b2), float(1 - b2), float(g["eps"])

    def _adam_state(self):
        """optimizer.state[p], created as torch's Adam._init_group does on its first step (non-capturable, non-fused)."""
        st = self.optimizer.state[self.adam_p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(self.adam_p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(self.adam_p, memory_format=torch.preserve_format)
        return st

    def _check_p(self, p):
        if self.optimizer is not None and p.data_ptr() != self.adam_p.data_ptr():
            raise ValueError("the Adam step updates the optimizer's own parameter; pass that tensor as p")

    def _pre_step(self, consts=None):
        """Host side of one step, before its launches (eager step, single-graph replay and _SplitGraph.replay alike): this
        rank's WER counters of the previous step go behind the gradient, and for Adam the step count is advanced and the
        step's scalars go to ``adam_scal``.  ``consts``: the (w1, beta2, omb2, eps) a graph captured by value."""
        self._apply_loss()
        if self._ring is None:
            return
        with self._ring.slot() as h:
            if self.collective and not self.device_wer:
                h[0], h[1] = self._wer_next
                self._wer_next = (0.0, 0.0)
                self.stats[ST_WER_ERR:ST_WER_REF + 1].copy_(h[0:2], non_blocking=True)
            if self.optimizer is not None:
                if consts is not None and self.adam_consts() != consts:
                    raise ValueError("Adam betas / eps changed after capture(); capture the step again")
                g = self.optimizer.param_groups[0]
                st = self._adam_state()
                if self.adam_p.grad is not self.adam_grad:
                    self.adam_p.grad = self.adam_grad
                st["step"] += 1                                                  # _multi_tensor_adam: steps on the CPU
                self.optimizer._opt_called = True   # what torch's wrapped optimizer.step() sets for the LR schedulers' order check
                h[2], h[3] = adam_scalars(g["lr"], g["betas"][0], g["betas"][1], st["step"].item())
                self.adam_scal.copy_(h[2:4], non_blocking=True)

    def _update(self, p, grad, n):
        """The update over ``n`` elements, on the current device: p += lr * sign(grad) (train.py:160-161), or the optimizer's
        Adam step (train.py:168-171: Adam minimises -direction * loss, grad = d(direction * loss))."""
        lib, st = _lib.lib(), _lib.stream_ptr()
        if self.optimizer is None:
            _lib.check(lib.paa_sign_step(_lib.ptr(p), _lib.ptr(grad), float(self.args.lr), n, st))
        else:
            w1, b2, omb2, eps = self.adam_consts()
            ast = self._adam_state()
            _lib.check(lib.paa_adam_step(_lib.ptr(p), _lib.ptr(grad), -1.0, _lib.ptr(ast["exp_avg"]), _lib.ptr(ast["exp_avg_sq"]),
                                         _lib.ptr(self.adam_scal), w1, b2, omb2, eps, _lib.ptr(self.adam_grad), n, st))

    # ---- capture ----------------------------------------------------------------------------------------------------
    def _replay_state(self):
        """The device tensors a step advances and the warm-up step of capture() hands back."""
        return [self.stats_log.cursor] if self.device_wer else []

    def _warm_up(self, p, clean, labels, logits_out, refs, lengths=None):
        """What capture() does before it opens a graph: fixes the buffers the graph will point into (-> labels, logits_out), runs
        one eager step on a side stream, as torch's capture rules require, and undoes it — ``p``, the optimizer state and its
        step count, the log cursor (the log holds replayed steps only) and the leaf's ``_replay_state`` are as before."""
        lab = None if labels is None else labels.to(device=self.dev, dtype=torch.int32).contiguous()      # None: the feature loss only
        self._alpha_captured = self.mask_alpha > 0
        if lengths is not None:
            self.set_lengths(lengths)
        if self.lengths_on:
            self._frames(clean.shape[0])                  # allocates the frame-count buffer outside the capture
        self._lengths_captured = self.lengths_on
        saved = None
        if self.optimizer is not None:
            self._check_p(p)
            ast = self._adam_state()
            saved = (p.detach().clone(), ast["exp_avg"].clone(), ast["exp_avg_sq"].clone(), ast["step"].clone())
        if logits_out is None:
            logits_out = torch.empty(clean.shape[0], self.model.frames, self.model.arch.vocab_size, device=self.dev)
        self._captured_buffers = (lab, logits_out)        # the graphs hold raw pointers: keep what capture() itself created alive
        if self.device_wer and refs is not None:
            self.set_refs(refs)
        state = [(t, t.clone()) for t in self._replay_state()]
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(s):
            self.step(p, clean, lab, logits_out=logits_out)
        torch.cuda.current_stream(self.dev).wait_stream(s)
        for t, t0 in state:
            t.copy_(t0)
        if saved is not None:
            torch.cuda.synchronize(self.dev)
            p.detach().copy_(saved[0])
            ast["exp_avg"].copy_(saved[1])
            ast["exp_avg_sq"].copy_(saved[2])
            ast["step"].copy_(saved[3])
        return lab, logits_out

    def _capture_body(self, p, clean, lab, logits_out):
        """``_body`` as ONE hipGraph -> (graph, result dict); with Adam the graph is wrapped (``_AdamGraph``)."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            r = self._body(p, clean, lab, logits_out=logits_out)
        return (g if self.optimizer is None else _AdamGraph(self, g)), r


class PgdStepper(_StepperCore):
    def __init__(self, model, args, length: int, interp=None, spl_thresh=None, group=None, force_collective=False,
                 optimizer=None, device_wer=False, canon=None, r_cap=None, log_cap=4096, p_length=None):
        """``device_wer``: count this step's word errors on the device and log every step's stats (module docstring); ``canon``
        is ``loss_helpers.canon_table(processor)`` (default: the built-in vocabulary), ``r_cap`` the width of the ``refs`` rows.
        ``force_collective``: run the packed all-reduce (and the global-statistics projection) even with a single rank —
        the way the one-GPU test box executes the RCCL branch (tests/test_gpu_rccl.py).  ``optimizer``: a torch.optim.Adam
        over the perturbation (``adam_unsupported`` is None); the step then applies its update instead of the sign step.
        ``length`` is the clip length L.  With placement on (module docstring) the perturbation has ``p_length`` samples (default:
        ``place.perturbation_length(args, L)``); with placement off it has L."""
        L = int(length)
        self.group, self.interp = group, interp
        self.world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world = torch.distributed.get_world_size(group)
        # refusals, before any launch or collective.  The stepper's own order (not chain.check's): the rooms' and the channel's
        # before the perturbation length is settled, placement's after it
        rir.check(args)
        channel.check(args)
        m = Modes.of(args)
        self.place_on, self.rir_on, self.chan_on, self.Lp = m.place_on, m.rir_on, m.chan_on, L
        if m.place_on:
            self.Lp = int(p_length) if p_length is not None else place.perturbation_length(args, L)
        elif p_length is not None and int(p_length) != L:
            raise ValueError(f"p_length {p_length} != clip length {L} needs placement on (perturbation_seconds)")
        place.check(args, L, self.Lp)
        modes.check(m, ("route",), Ctx(self.world))
        self.collective = self.world > 1 or bool(force_collective)
        if self.collective and not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            raise RuntimeError("force_collective needs an initialised torch.distributed process group")
        super().__init__(model, args, L, interp, spl_thresh, optimizer, device_wer, canon, r_cap, log_cap, 1, self.Lp)
        self.need_clean_stats = self.collective and any(n in ("snr", "tv") for n in self.norms)
        self.packed = torch.zeros(self.Lp + N_STATS, dtype=torch.float32, device=self.dev)
        self.grad = self.packed[: self.Lp].view(1, self.Lp)
        self.stats = self.packed[self.Lp:]
        if self.place_on or self.rir_on or self.chan_on:          # the playback chain; the attribute is absent with all three off
            rank = torch.distributed.get_rank(self.group) if self.world > 1 else 0
            self.placed = chain.PlaybackChain(args, model, self.Lp, place.STREAM_TRAIN, True, rank, L)

    def _check_adam_shape(self):
        if self.adam_p.numel() != self.Lp:
            raise ValueError(f"optimizer parameter has {self.adam_p.numel()} elements, expected {self.Lp}")

    # ---- the playback chain: placement, room responses, the channel ----------------------------------------------------
    @property
    def placer(self):
        return self.placed.placer

    @property
    def reverb(self):
        return self.placed.reverb

    @property
    def chan(self):
        return self.placed.chan

    _SITES = {"placer": ("place_on", "placement off (perturbation_seconds / place_shift / place_gain_db)"),
              "reverb": ("rir_on", "room responses off (rir_bank)"),
              "chan": ("chan_on", "the playback channel off (drift_ppm / noise_snr_db)")}

    def _site(self, name):
        """The chain's site ``name``; raises when the stepper was built with its mode off."""
        on, off = self._SITES[name]
        if not getattr(self, on):
            raise RuntimeError(f"the stepper was built with {off}")
        return getattr(self.placed, name)

    def set_placement(self, shift, gain=None):
        """Explicit per-clip shifts (and gains, default 1) instead of the draw, from the next step on (stream-ordered copy into the
        fixed buffers); ``set_placement(None)`` returns to drawing.  A captured graph keeps the form it was captured with."""
        self._site("placer").set_placement(shift, gain)

    def set_rooms(self, index):
        """The same for per-clip room indices."""
        self._site("reverb").set_rooms(index)

    def set_channel(self, ratio, snr_db=None):
        """The same for per-clip clock ratios (and noise SNRs in dB).  The noise samples keep their own counter and stay fresh."""
        self._site("chan").set_channel(ratio, snr_db)

    def set_place_step(self, n: int):
        """Device step counter of the next placement draw (resume, tests)."""
        self._site("placer").set_step(n)

    def set_rir_step(self, n: int):
        """... of the next room draw."""
        self._site("reverb").set_step(n)

    def set_chan_step(self, n: int):
        """... of the next channel draw and the next noise."""
        self._site("chan").set_step(n)

    @property
    def clip_base(self):
        """Global id of this rank's first clip in the draws' counters (default rank * model.max_batch); assignable per step.  A
        captured graph holds the value it was captured with."""
        if not (self.rir_on or self.chan_on):
            self._site("placer")
        return self.placed.clip_base

    @clip_base.setter
    def clip_base(self, v):
        if not (self.rir_on or self.chan_on):
            self._site("placer")
        self.placed.clip_base = v

    def _replay_state(self):
        return super()._replay_state() + (self.placed.counters() if self.place_on or self.rir_on or self.chan_on else [])

    # ---- bookkeeping carried by the packed vector -------------------------------------------------------------
    def set_wer_counts(self, errors: float, ref_words: float):
        """Host-side WER counters of the PREVIOUS step (train.py:149-153): the next ``step`` writes them behind the
        gradient, so its all-reduce sums them over ranks; read the global sums from ``stats[3:5]`` afterwards."""
        self._wer_next = (float(errors), float(ref_words))

    # ---- the two halves of a step (everything before / after the collective) ----------------------------------
    def _pre(self, p, clean, labels, want_logits=True, logits_out=None):
        B = clean.shape[0]
        out = {"grad": self.grad, "stats": self.stats}
        if logits_out is not None:
            out["logits"] = logits_out
        placed = self.place_on or self.rir_on or self.chan_on      # chain.PlaybackChain: one gradient row per clip, then their adjoint into self.grad
        if placed:
            out["grad"] = self.placed.placer.grad_rows[:B]
        if self.modes.feature_on:          # the reference follows the step's clean batch: inside the launch sequence, so inside a graph
            self._feature_reference(clean)
        r = self.model.fwd_bwd(clean, self.placed.rows(p, B, clean) if placed else p, labels, self.direction, want_grad=True,
                               want_logits=want_logits, out=out)
        if placed:
            self.placed.reduce(B, self.grad)
            r["grad_rows"], r["grad"] = r["grad"], self.grad
        if self.mask_alpha > 0:
            self._masking_loss(p, clean, self.grad)
            r["masking_loss"] = self.stats[ST_MASK_LOSS]
        if self.device_wer:
            self._wer(r["logits"], B)
        if self.need_clean_stats:
            with torch.cuda.device(self.dev):
                _lib.check(_lib.lib().paa_batch_stats(self.proj.h, _lib.ptr(clean), B, self.L, _lib.ptr(self.stats[ST_SQ:ST_TV + 1]),
                                                      _lib.ptr(self.stats[ST_CLIPS:ST_CLIPS + 1]), _lib.stream_ptr()))
        return r

    def _post(self, p, clean):
        lib, Lp, B = _lib.lib(), self.Lp, clean.shape[0]
        if Lp != self.L:                    # a perturbation of its own length: nothing pairs it with the clean samples
            clean, B = None, 0
        with torch.cuda.device(self.dev):
            st = _lib.stream_ptr()
            self._update(p, self.grad, Lp)
            for n, prm in zip(self.norms, self._prm):                                                   # train.py:162
                if self.need_clean_stats and n in ("snr", "tv"):
                    _lib.check(lib.paa_project_ext(self.proj.h, prm, _lib.ptr(p), 1, _lib.ptr(self.stats[ST_SQ:ST_TV + 1]),
                                                   _lib.ptr(self.stats[ST_CLIPS:ST_CLIPS + 1]), 0.0, Lp, st))
                else:
                    _lib.check(lib.paa_project(self.proj.h, prm, _lib.ptr(p), 1, _lib.ptr(clean), B, Lp, st))
        if self.device_wer:
            self.stats_log.push(self.stats)

    def step(self, p: torch.Tensor, clean: torch.Tensor, labels: torch.Tensor, want_logits=True, logits_out=None, refs=None,
             lengths=None):
        """In place on ``p`` (1, L).  Returns dict(loss: 0-d device tensor, summed over ALL ranks, logits).  ``refs``
        (device_wer only): this batch's reference rows, copied to the fixed buffer first (``set_refs``); None keeps what the
        buffer holds.  ``lengths``: this batch's true sample counts (``set_lengths``); None leaves the model as it is."""
        if refs is not None:
            self.set_refs(refs)
        if lengths is not None:
            self.set_lengths(lengths)
        p = runtime.as_f32_cuda(p, "p")
        clean = runtime.as_f32_cuda(clean, "clean_audio")
        if p.numel() != self.Lp or clean.shape[-1] != self.L:
            raise ValueError(f"Loaded perturbation length {p.numel()} / clip length {clean.shape[-1]} != expected "
                             f"{self.Lp if self.place_on else self.L}" + (f" / {self.L}" if self.place_on else ""))
        self._check_p(p)
        self._fit_proj(clean.shape[0])
        self._pre_step()
        return self._body(p, clean, labels, want_logits, logits_out)

    def _fit_proj(self, B):
        """The masking norm and the masking loss keep one bound per clip of the batch: grow the projection workspace to the
        batch (allocates, so it happens in an eager step; capture() runs one first)."""
        if (self.modes.masking_norm or self.mask_alpha > 0) and self.proj.max_batch < B:
            self.proj = runtime.get_proj(self.args, self.dev, B, self.L, self.interp)

    def _body(self, p, clean, labels, want_logits=True, logits_out=None):
        r = self._pre(p, clean, labels, want_logits, logits_out)
        if self.collective:
            torch.distributed.all_reduce(self.packed, op=torch.distributed.ReduceOp.SUM, group=self.group)
        self._post(p, clean)
        r["loss"] = self.stats[ST_LOSS]
        return r

    def capture(self, p, clean, labels, logits_out=None, refs=None, lengths=None):
        """Capture one step on fixed buffers into hipGraphs (the launch sequence allocates nothing and never
        synchronises, so it is capturable as is).  With device_wer, ``refs`` fills the fixed reference buffer (refresh it with
        ``set_refs`` before a replay) and the warm-up step's log row is taken back: the log holds replayed steps only.  Returns
        (graph, result dict); ``graph.replay()`` re-runs the step in place on ``p`` with whatever ``clean`` / ``labels`` currently
        hold.  With several ranks the halves before and after the collective are two graphs and the all-reduce runs between
        their replays.

        With Adam the result is always an object with ``replay()`` (the step's scalars are pushed before each replay), betas
        and eps are captured by value (``replay()`` raises ValueError once they change), and the warm-up step is undone:
        ``p``, the optimizer state and the step count are as before the call.

        The graphs hold raw pointers into this stepper's buffers (and into ``p``, ``clean`` and the labels): a plain
        ``torch.cuda.CUDAGraph`` does not keep them alive, so the caller keeps the stepper and those tensors for as long as it
        replays the graph.  A freed block is handed to later allocations, and labels read as another tensor's bits index the
        logits out of bounds.

        With placement the draw is inside the graph (the first one of the split form) and the warm-up step's draw is taken back:
        the device step counter is as before the call, so the first replay draws what the first eager step would have.

        ``lengths`` as ``step``; the graph reads the model's length buffer, so ``set_lengths`` before a replay changes the clips'
        lengths without re-capture."""
        lab, logits_out = self._warm_up(p, clean, labels, logits_out, refs, lengths)
        if not self.collective:
            return self._capture_body(p, clean, lab, logits_out)
        # No collective may be in flight while a capture is open (the process group's watchdog thread polls its events), and the
        # captures only guard THIS thread's launches: the RCCL call between them runs eagerly.
        torch.cuda.synchronize(self.dev)
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, capture_error_mode="thread_local"):
            r = self._pre(p, clean, lab, True, logits_out)
        torch.distributed.all_reduce(self.packed, op=torch.distributed.ReduceOp.SUM, group=self.group)
        torch.cuda.synchronize(self.dev)
        with torch.cuda.graph(g2, capture_error_mode="thread_local"):
            self._post(p, clean)
        r["loss"] = self.stats[ST_LOSS]
        return _SplitGraph(self, g1, g2), r


class _AdamGraph:
    """Single-graph Adam step: replay() = host scalars of the step, then the captured launches."""

    def __init__(self, stepper, g):
        self.stepper, self.g = stepper, g
        self.consts = stepper.adam_consts()

    def replay(self):
        self.stepper._pre_step(self.consts)
        self.g.replay()


class _SplitGraph:
    """replay() = pre-collective graph, all-reduce of the packed vector, post-collective graph."""

    def __init__(self, stepper, g1, g2):
        self.stepper, self.g1, self.g2 = stepper, g1, g2
        self.consts = stepper.adam_consts() if stepper.optimizer is not None else None

    def replay(self):
        self.stepper._pre_step(self.consts)
        self.g1.replay()
        torch.distributed.all_reduce(self.stepper.packed, op=torch.distributed.ReduceOp.SUM, group=self.stepper.group)
        self.g2.replay()
