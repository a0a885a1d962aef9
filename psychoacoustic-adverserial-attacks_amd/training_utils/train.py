"""Same call surface as the reference's ``src/training_utils/train.py``:
``perturbation_constraint(p, clean_audio, args, interp, spl_thresh)`` and
``train_epoch(args, train_data_loader, p, model, epoch, processor, interp, wer_metric, spl_thresh, optimizer)``
— executed by libpaa_hip.so."""
from __future__ import annotations

import logging
import time
from dataclasses import dataclass
from typing import Iterable

import torch

from .. import _lib, runtime
from ..core import loss_helpers
from . import chain, modes
from .modes import Ctx, Modes
from .pgd import FREQ_NORMS, PgdStepper, adam_unsupported, batch_lengths

logger = logging.getLogger(__name__)


@dataclass(frozen=True)
class TrainEpochResult:          # train.py:15-19
    p: torch.Tensor
    avg_ctc: float
    avg_wer: float
    avg_masking_loss: float = None        # mean over the steps of sum_b l_b (masking_loss_alpha > 0 only)


def _avg(values: Iterable[float]) -> float:
    vals = list(values)
    return sum(vals) / max(len(vals), 1)


def global_wer_per_step(counts, device, group=None):
    """Data-parallel runs: ``counts`` = this rank's [(word errors, reference words)] per step.  The WER the reference would
    report for the GLOBAL batch of a step is sum_r errors / sum_r words (jiwer is corpus-level within a batch), so the
    per-step counts of all ranks are summed by ONE small all-reduce at the end of the epoch (every rank runs the same
    number of steps — the step's own all-reduce already requires that)."""
    import torch.distributed as dist
    t = torch.tensor(counts, dtype=torch.float64, device=device).reshape(-1, 2)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    t = t.cpu()
    return [float(e) / max(float(w), 1.0) for e, w in t.tolist()]


_host_route_logged = set()


def device_wer_canon(args, processor, wer_metric, where: str):
    """The canon table when ``where`` (train_epoch / evaluate / attack_clips) may count word errors on the device, else None —
    the host route, with its reason logged once: the flag is off (silently), a ``wer_metric`` object is given (jiwer applies
    its own transforms), or the vocabulary is not one character per token (``loss_helpers.canon_table``)."""
    if not getattr(args, "device_wer", False):
        return None
    why, canon = None, None
    if wer_metric is not None:
        why = "a wer_metric object is given"
    else:
        canon = loss_helpers.canon_table(processor)
        if canon is None:
            why = "the vocabulary is not one character per token"
    if why is not None:
        log_host_route(where, why)
    return canon


def log_host_route(where: str, why: str):
    if (where, why) not in _host_route_logged:
        _host_route_logged.add((where, why))
        logger.warning("%s: --device_wer falls back to the host WER path: %s", where, why)


def wer_of_rows(rows):
    """Per-step WER of stats-log rows: errors / max(reference words, 1), both small integers held exactly in float32."""
    return [float(e) / max(float(w), 1.0) for e, w in rows[:, [3, 4]].tolist()]


def perturbation_constraint(p: torch.Tensor, clean_audio, args, interp, spl_thresh) -> torch.Tensor:
    """train.py:69-99.  Returns a new tensor; ``p`` is left untouched.  ``args.norm_type`` may be a
    '+'-joined list (extension, applied in the written order)."""
    m = Modes.of(args)
    norms = m.norms
    for n in norms:
        if n not in _lib.NORM_IDS:
            raise ValueError(f"Unknown norm_type: {n!r}")                                   # train.py:98
        if n == "snr" and clean_audio is None:
            raise ValueError("SNR projection requires clean_audio ro compare to")           # train.py:91
        if n == "tv" and clean_audio is None:
            raise ValueError("TV projection can benefit from clean_audio for bounds")       # train.py:95
        if n == "masking" and clean_audio is None:
            raise ValueError("masking projection requires clean_audio")
    src = runtime.as_f32_cuda(p.detach(), "p")
    q = torch.empty_like(src)
    rows, L = (q.shape[0], q.shape[1]) if q.dim() == 2 else (1, q.shape[0])
    clean = None if clean_audio is None else runtime.as_f32_cuda(clean_audio, "clean_audio")
    if clean is not None and clean.shape[-1] != L:
        raise ValueError(f"clean_audio length {clean.shape[-1]} != perturbation length {L}")
    # the masking norm keeps one bound per clean clip before their minimum: the workspace holds the whole batch
    nb_ws = clean.shape[0] if clean is not None and clean.dim() == 2 and m.masking_norm else 0
    pr = runtime.get_proj(args, q.device, max(rows, nb_ws), L, interp)
    out_len = L
    with torch.cuda.device(q.device):
        for i, n in enumerate(norms):
            prm = runtime.params_of(args, n)
            if n == "max_phon":
                pr.set_spl_thresh(spl_thresh)
            nb = 0 if clean is None else clean.shape[0]
            if i == 0:       # the reference's functions return a new tensor: out of place from p (one fused launch for the FFT norms)
                _lib.check(_lib.lib().paa_project_to(pr.h, prm, _lib.ptr(src), _lib.ptr(q), rows, _lib.ptr(clean),
                                                     nb, L, _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().paa_project(pr.h, prm, _lib.ptr(q), rows, _lib.ptr(clean), nb, L, _lib.stream_ptr()))
            if n in FREQ_NORMS and clean is None:
                out_len = pr.hop * (L // pr.hop)        # iSTFT length hop*(T-1); no _align_to without clean audio
    return q if out_len == L else q[..., :out_len]


def adam_route(optimizer, world: int) -> str:
    """Which update the Adam branch runs: "device" (paa_adam_step inside PgdStepper's launch sequence) for the plain
    torch.optim.Adam build.py:352-359 creates, "eager" (torch's own optimizer.step) for any other optimizer on one rank.
    With several ranks only the device step exists: NotImplementedError names the option it does not cover."""
    why = adam_unsupported(optimizer)
    if why is not None and world > 1:          # about the optimizer object, not the mode flags: not in modes.RULES
        raise NotImplementedError(f"the data-parallel Adam step does not implement {why}; use the defaults of "
                                  "torch.optim.Adam(lr=...) or a single rank")
    return "device" if why is None else "eager"


def train_epoch(args, train_data_loader, p: torch.Tensor, model, epoch: int, processor, interp, wer_metric,
                spl_thresh, optimizer) -> TrainEpochResult:
    """train.py:103-182.  ``model`` is a ``paa_amd.model.PaaModel``."""
    ctc_scores, wer_scores, wer_counts, times = [], [], [], []
    logger.info("starting epoch: %d", epoch)
    if args.optimizer_type not in ("pgd", "adam"):
        raise NotImplementedError(f"Optimization type not implemented: {args.optimizer_type!r}")   # train.py:177
    if args.optimizer_type == "adam" and optimizer is None:
        raise ValueError("Adam optimizer selected but optimizer is None")                          # train.py:167
    Lp = p.shape[-1]
    m = Modes.of(args)
    L = int(model.length) if m.place_on else Lp          # placement: p has a length of its own (place.py)
    world = 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        world = torch.distributed.get_world_size()
    # The eager torch chain stays only for a one-rank run whose optimizer the device step does not implement (weight decay,
    # AMSGrad, ...): there it is what the reference runs, and the data-parallel machinery has nothing to add.
    eager_adam = args.optimizer_type == "adam" and adam_route(optimizer, world) == "eager"
    modes.check(m, ("alpha_eager",), Ctx(world, eager_adam))          # refusals: before any launch or collective
    chain.check(args, L, Lp, eager_adam)
    modes.check(m, modes.LENGTHS + ("len_eager",), Ctx(world, eager_adam))
    step_opt = optimizer if args.optimizer_type == "adam" and not eager_adam else None
    mask_alpha, lengths_mode = m.alpha, m.lengths_on
    mask_scores = []
    canon = None if eager_adam else device_wer_canon(args, processor, wer_metric, "train_epoch")
    if eager_adam and m.device_wer:
        log_host_route("train_epoch", "the optimizer runs torch's own step")
    stepper = getattr(model, "_stepper", None)
    if stepper is None or stepper.args is not args or stepper.L != L or stepper.Lp != Lp or stepper.optimizer is not step_opt \
            or stepper.device_wer != (canon is not None):
        stepper = PgdStepper(model, args, L, interp, spl_thresh, optimizer=step_opt, device_wer=canon is not None, canon=canon,
                             p_length=Lp)
        model._stepper = stepper
        if stepper.place_on or stepper.rir_on or stepper.chan_on:
            # a resumed run goes on drawing where the epochs before it stopped, not from step 0 again
            stepper.placed.set_step(int(epoch) * len(train_data_loader))
    if not lengths_mode and stepper.lengths_on:
        stepper.set_lengths(None)             # a model left in the length mode by an earlier caller: padded means padded
    if canon is not None:
        return _train_epoch_device(args, train_data_loader, p, stepper, processor, mask_alpha, lengths_mode)
    blank = int(model.arch.pad_token_id)
    for batch in train_data_loader:
        clean_audio, target_texts, lengths = batch_lengths(batch, lengths_mode)
        t0 = time.perf_counter()
        clean_audio = clean_audio.to(args.device, torch.float32, non_blocking=True).contiguous()   # train.py:129
        labels = loss_helpers.make_labels(target_texts, processor, args, len(clean_audio))
        if args.optimizer_type == "pgd":
            if isinstance(p, torch.nn.Parameter) or p.requires_grad:
                p = p.detach()
            r = stepper.step(p, clean_audio, labels, lengths=lengths)
        elif not eager_adam:
            r = stepper.step(p.data, clean_audio, labels, lengths=lengths)     # p.grad = -grad, as train.py:170 leaves it
        else:
            if p.dtype != torch.float32 or not p.is_cuda:
                raise TypeError(f"the Adam branch needs a float32 perturbation on the GPU, got {p.dtype} on {p.device}")
            stepper._apply_loss()          # --loss_type, as the device step applies it
            if stepper.modes.feature_on:
                stepper._feature_reference(clean_audio)
            r = model.fwd_bwd(clean_audio, p.data, labels, stepper.direction)
            optimizer.zero_grad(set_to_none=True)
            p.grad = -r["grad"].view_as(p)          # gradient of (-direction * loss), train.py:170
            optimizer.step()
            with torch.no_grad():
                p.data = perturbation_constraint(p.data, clean_audio, args, interp, spl_thresh)   # train.py:172-175
        ctc_scores.append(float(r["loss"].item()))                                   # train.py:146
        if mask_alpha > 0:
            mask_scores.append(float(r["masking_loss"].item()))
        frames = model.frame_counts(len(clean_audio)) if lengths_mode else None
        pred_texts, ref_texts = loss_helpers.wer_texts(r["logits"], target_texts, processor, frames, blank)   # train.py:149-153
        e, w = loss_helpers.wer_counts(pred_texts, ref_texts)
        wer_counts.append((e, w))
        stepper.set_wer_counts(e, w)          # rides behind the next step's gradient (stats[3:5] = sums over ranks)
        wer_scores.append(float(wer_metric.compute(predictions=pred_texts, references=ref_texts)) if wer_metric is not None
                          else e / max(w, 1))
        times.append(time.perf_counter() - t0)
    if stepper.world > 1:                     # the loss in stats[0] is already the global batch's; make the WER global too
        wer_scores = global_wer_per_step(wer_counts, stepper.dev, stepper.group)
    return TrainEpochResult(p=p, avg_ctc=_avg(ctc_scores), avg_wer=_avg(wer_scores),
                            avg_masking_loss=_avg(mask_scores) if mask_alpha > 0 else None)


def _train_epoch_device(args, train_data_loader, p, stepper, processor, mask_alpha, lengths_mode=False) -> TrainEpochResult:
    """train_epoch with the WER counted on the device (--device_wer): the loop body launches the step and nothing else — no
    .item(), no id download, no host decode — and the per-step CTC loss, masking loss and word counters come back in ONE
    readback of the stepper's stats log at the end of the epoch (already global sums with several ranks: they rode the step's
    all-reduce).  A batch whose references do not fit the device rows (``encode_refs`` is None) takes the host route for its
    WER, one rank only."""
    rows, host_wer, n = [], {}, 0
    stepper.stats_log.cursor.zero_()          # stream-ordered: rows a caller left unread do not count as this epoch's
    for batch in train_data_loader:
        clean_audio, target_texts, lengths = batch_lengths(batch, lengths_mode)
        clean_audio = clean_audio.to(args.device, torch.float32, non_blocking=True).contiguous()   # train.py:129
        labels = loss_helpers.make_labels(target_texts, processor, args, len(clean_audio))
        refs = loss_helpers.encode_refs(target_texts, stepper.r_cap)
        fits = refs is not None
        if not fits:
            if stepper.world > 1:
                raise NotImplementedError(f"--device_wer with several ranks: a reference needs more than {stepper.r_cap} "
                                          "entries; run without the flag")
            log_host_route("train_epoch", f"a reference needs more than {stepper.r_cap} entries")
            refs = loss_helpers.encode_refs([""] * len(target_texts), stepper.r_cap)
        if args.optimizer_type == "pgd":
            if isinstance(p, torch.nn.Parameter) or p.requires_grad:
                p = p.detach()
            r = stepper.step(p, clean_audio, labels, refs=refs, lengths=lengths)
        else:
            r = stepper.step(p.data, clean_audio, labels, refs=refs, lengths=lengths)   # p.grad = -grad, as train.py:170 leaves it
        if not fits:
            frames = stepper.model.frame_counts(len(clean_audio)) if lengths_mode else None
            host_wer[n] = loss_helpers.wer_counts(*loss_helpers.wer_texts(r["logits"], target_texts, processor, frames,
                                                                          int(stepper.model.arch.pad_token_id)))
        n += 1
        if n % stepper.stats_log.cap == 0:
            rows.append(stepper.read_log())
    rows.append(stepper.read_log())
    rows = torch.cat(rows, dim=0)
    if rows.shape[0] != n:
        raise RuntimeError(f"the stats log holds {rows.shape[0]} rows after {n} steps")
    wer_scores = wer_of_rows(rows)
    for i, (e, w) in host_wer.items():
        wer_scores[i] = e / max(w, 1)
    return TrainEpochResult(p=p, avg_ctc=_avg(rows[:, 0].tolist()), avg_wer=_avg(wer_scores),
                            avg_masking_loss=_avg(rows[:, 6].tolist()) if mask_alpha > 0 else None)
