"""Evaluation loop — reference ``src/training_utils/evaluation.py:5-31`` on the HIP forward path.
Note the reference adds ``p`` WITHOUT clamping here (evaluation.py:16), unlike the training step."""
from __future__ import annotations

import torch

from ..core import loss_helpers
from . import chain, channel, modes, place, rir
from .build import batch_lengths
from .scoring_helpers import Scores


class _PlacedEval:
    """evaluate(perturbed=True) with placement on: every batch sees the perturbation at a drawn placement (Philox stream 1, the
    step counter restarting at 0 in every evaluate call, so every evaluation sees the same placements and epochs compare).  With
    room responses on (training_utils/rir.py) the rows then pass through rooms drawn the same way: every evaluation hears the same
    rooms; with placement itself off the rows are the perturbation at shift 0 and gain 1.  With the playback channel on
    (training_utils/channel.py) the rows are drifted and noise is added the same way: the draw's and the noise's counters restart
    at 0 with this object, so every evaluation hears the same channels and the same noise."""

    def __init__(self, args, model, pp):
        rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
        place.check(args, int(model.length), pp.numel())
        place.shift_on(args), place.gain_db(args)          # rooms alone still place: these two flags are read before the rooms'
        rir.check(args)
        channel.check(args)
        self.pp, self.placed = pp, chain.PlaybackChain(args, model, pp.numel(), place.STREAM_EVAL, False, rank)

    def rows(self, B, clean=None):
        return self.placed.rows(self.pp, B, clean)


def _pert(pp, B, clean=None):
    """The perturbation operand of model.forward for a batch of B clips: the (1, L) row, placed rows, or None.  ``clean``: the
    batch itself, whose level scales the channel's noise."""
    return pp.rows(B, clean) if isinstance(pp, _PlacedEval) else pp


def _set_lengths(model, lengths, B):
    """This batch's true sample counts into the model's length buffer -> its frame counts T_b (device int32), or None when the
    batch carries none (--clip_lengths padded)."""
    if lengths is None:
        return None
    model.set_lengths(lengths)
    return model.frame_counts(B)


def _evaluate_device(args, eval_data_loader, pp, model, processor, canon, lengths_mode=False) -> Scores:
    """evaluate with the WER counted on the device (--device_wer): forward -> paa_argmax_ids + paa_wer_counts -> one row of
    [CTC loss, ..., word errors, reference words] appended to a device log; no .item() and no host decode in the loop, ONE
    readback at the end (and, sharded over ranks, one all-reduce of the rows instead of two).  A batch whose references do not fit
    the device rows takes the host route for its counters."""
    from .pgd import N_STATS, ST_LOSS, ST_WER_ERR, ST_WER_REF, StatsLog
    from .train import log_host_route, wer_of_rows
    dev = model.device
    blank = int(model.arch.pad_token_id)
    log = StatsLog(dev, 1024, N_STATS)
    st = torch.zeros(N_STATS, dtype=torch.float32, device=dev)
    canon = canon.to(dev)
    chunks, host, n = [], {}, 0
    for batch in eval_data_loader:
        data, target_texts, lengths = batch_lengths(batch, lengths_mode)
        if len(target_texts) == 0:           # an empty shard of a short global batch: a row of zeros for the all-reduce
            st.zero_()
        else:
            data = data.to(args.device, torch.float32).contiguous()
            labels = loss_helpers.make_labels(target_texts, processor, args, len(data))
            frames = _set_lengths(model, lengths, len(data))
            r = model.forward(data, _pert(pp, len(data), data), labels, clamp=False)
            st[ST_LOSS].copy_(r["loss"])
            refs = loss_helpers.encode_refs(target_texts)
            if refs is None:
                log_host_route("evaluate", f"a reference needs more than {loss_helpers.R_CAP} entries")
                host[n] = loss_helpers.wer_counts(*loss_helpers.wer_texts(r["logits"], target_texts, processor, frames, blank))
                st[ST_WER_ERR:ST_WER_REF + 1].zero_()
            else:
                loss_helpers.wer_counts_device(r["logits"], refs, canon, sums=st[ST_WER_ERR:ST_WER_REF + 1], frames=frames,
                                               blank=blank)
        log.push(st)
        n += 1
        if n % log.cap == 0:
            chunks.append(log.read())
    chunks.append(log.read())
    rows = torch.cat(chunks, dim=0)
    for i, (e, w) in host.items():
        rows[i, ST_WER_ERR], rows[i, ST_WER_REF] = float(e), float(w)
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        rows = rows.to(dev, torch.float64)
        torch.distributed.all_reduce(rows)
        rows = rows.cpu()
    ctc_scores, wer_scores = rows[:, ST_LOSS].tolist(), wer_of_rows(rows)
    avg_ctc = sum(ctc_scores) / len(ctc_scores) if ctc_scores else float("inf")
    avg_wer = sum(wer_scores) / len(wer_scores) if wer_scores else float("inf")
    return Scores(ctc=avg_ctc, wer=avg_wer)


def evaluate(args, eval_data_loader, p, model, processor, wer_metric, perturbed=False, epoch_number=-1) -> Scores:
    m = modes.check(modes.Modes.of(args), modes.LENGTHS)          # refusals of --clip_lengths true: before any launch or collective
    lengths_mode = m.lengths_on
    ctc_scores, wer_scores, counts = [], [], []
    pp = None
    if perturbed and isinstance(p, torch.Tensor):
        pp = p.detach().to(model.device, torch.float32).reshape(1, -1).contiguous()
        if m.place_on or m.rir_on or m.chan_on:
            pp = _PlacedEval(args, model, pp)
    if not lengths_mode and model.lengths_on:
        model.set_lengths(None)                      # padded means padded, whatever an earlier caller left behind
    blank = int(model.arch.pad_token_id)
    if m.device_wer:
        from .train import device_wer_canon
        canon = device_wer_canon(args, processor, wer_metric, "evaluate")
        if canon is not None:
            return _evaluate_device(args, eval_data_loader, pp, model, processor, canon, lengths_mode)
    for batch in eval_data_loader:
        data, target_texts, lengths = batch_lengths(batch, lengths_mode)
        if len(target_texts) == 0:           # an empty shard of a short global batch (build.shard_batches): zeros for the all-reduce
            ctc_scores.append(0.0); wer_scores.append(0.0); counts.append((0, 0))
            continue
        data = data.to(args.device, torch.float32).contiguous()
        labels = loss_helpers.make_labels(target_texts, processor, args, len(data))
        frames = _set_lengths(model, lengths, len(data))
        r = model.forward(data, _pert(pp, len(data), data), labels, clamp=False)
        ctc_scores.append(float(r["loss"].item()))
        pred_texts, ref_texts = loss_helpers.wer_texts(r["logits"], target_texts, processor, frames, blank)
        e, w = loss_helpers.wer_counts(pred_texts, ref_texts)
        counts.append((e, w))
        wer_scores.append(float(wer_metric.compute(predictions=pred_texts, references=ref_texts)) if wer_metric is not None
                          else e / max(w, 1))
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        # sharded evaluation: CTC loss is a sum over clips and WER is corpus-level within a batch, so the global batch's
        # scores are the sums over ranks (one small all-reduce per evaluation)
        from .train import global_wer_per_step
        t = torch.tensor(ctc_scores, dtype=torch.float64, device=model.device)
        torch.distributed.all_reduce(t)
        ctc_scores = t.cpu().tolist()
        wer_scores = global_wer_per_step(counts, model.device)
    avg_ctc = sum(ctc_scores) / len(ctc_scores) if ctc_scores else float("inf")
    avg_wer = sum(wer_scores) / len(wer_scores) if wer_scores else float("inf")
    return Scores(ctc=avg_ctc, wer=avg_wer)
