"""Per-clip (per-utterance) attack entry point: every clip of a split gets its own perturbation delta_b, crafted with
``--pgd_steps`` device steps (training_utils/clip_attack.ClipStepper) under the same constraint sets as the universal
runner, then evaluated clean and adversarial.

    python -m paa_amd.attack_clips --norm_type snr --snr_db 40 --pgd_steps 20 [--split test] [--data_dir DIR]

Writes ``clip_results.json`` (one record per clip, then the summary means) and int16 wavs of the first
``--num_items_to_inspect`` adversarial clips into the run directory.  Launched with several ranks (WORLD_SIZE / RANK), the
clips of every global batch are sharded over the ranks (build.shard_batches), each rank attacks its shard without any
collective, and one gather after the last batch brings the records to rank 0, which writes the file.

``--bound_search shrink`` answers "how small a perturbation makes this clip fall?": the moment a clip's attack
succeeds its delta is remembered and its bound is multiplied by ``--search_shrink``; the record then describes the smallest
successful delta (``found``, ``found_step``, ``bound_scale``, ``last_scale``), or the last iterate of a clip that never fell.

``--loss_type margin`` (targeted attacks): the steps optimise the alignment-margin loss, which is zero exactly when
the greedy decode is the target — the search's success test.  The step's ``loss`` then holds the margin loss; the records'
``clean_ctc`` / ``final_ctc`` stay CTC.
"""
from __future__ import annotations

import copy
import json
import math
import os
import sys

import torch

from .core import iso, loss_helpers
from .core.masking import masking_loss
from .training_utils import build, modes, parser, save
from .training_utils.clip_attack import ClipStepper, clip_nll, compose_rows, init_rows, project_rows

SPLITS = ("test", "val", "train")
RECORD_FIELDS = ("index", "clean_wer", "adv_wer", "clean_ctc", "final_ctc", "l2", "linf", "snr_db")
TARGET_FIELD = "target_wer"
MASK_FIELD = "final_masking_loss"          # l_b(delta_b) of the finished perturbation (masking_loss_alpha > 0 only)
LENGTH_FIELD = "length"                     # the clip's true sample count (--clip_lengths true only)
SUMMARY_FIELDS = ("clean_wer", "adv_wer", "final_ctc", "l2", "linf", "snr_db")
# --bound_search shrink only: found (the step's own counters said "success" at least once), the step of the reported delta (-1: not
# found), the scale that delta satisfies (best_scale, or the last scale when not found) and the scale the search ended at
SEARCH_FIELDS = ("found", "found_step", "bound_scale", "last_scale")


def create_arg_parser():
    p = parser.create_arg_parser()
    p.add_argument("--pgd_steps", type=int, default=100, help="per-clip attack: device steps per batch")
    p.add_argument("--split", type=str, choices=list(SPLITS), default="test", help="per-clip attack: the split attacked")
    p.add_argument("--bound_search", type=str, choices=["off", "shrink"], default="off",
                   help="shrink: the moment a clip's attack succeeds, keep that perturbation and multiply the clip's bound by "
                        "--search_shrink; the record reports the smallest successful perturbation")
    p.add_argument("--search_shrink", type=float, default=0.8, help="bound search: factor applied to a clip's bound on success, in (0, 1)")
    p.add_argument("--search_floor", type=float, default=0.01, help="bound search: smallest bound scale, in (0, 1]")
    p.add_argument("--search_success_wer", type=float, default=0.5,
                   help="bound search, untargeted: success is per-clip WER >= this (rounded to thousandths); targeted success is "
                        "always the target transcript exactly")
    return p


def clip_batches(batches, rank: int = 0, world: int = 1):
    """Global batches (x (n, L), texts[, lengths]) of a split -> this rank's shards as (x, texts, global clip indices[,
    lengths]).  The index of a clip is its position in the split, whatever the batch size or the number of ranks."""
    tagged, first = [], 0
    for batch in batches:
        x, texts, lengths = build.unpack_batch(batch)
        idx = list(range(first, first + len(texts)))
        first += len(texts)
        tagged.append((x, list(zip(idx, texts))) if lengths is None else (x, list(zip(idx, texts)), lengths))
    out = []
    for shard in build.shard_batches(tagged, rank, world, keep_empty=True):
        x, pairs, lengths = build.unpack_batch(shard)
        if len(pairs):
            item = (x, [t for _, t in pairs], [i for i, _ in pairs])
            out.append(item if lengths is None else item + (lengths,))
    return out


def split_batches(args, world: int = 1):
    """The split ``args.split`` of build.create_data_loaders as global batches of ``batch_size * world`` clips, and the
    clip length."""
    g = copy.copy(args)
    g.batch_size = int(args.batch_size) * world
    tr, ev, te, length = build.create_data_loaders(g)
    return {"train": tr, "val": ev, "test": te}[args.split], length


def gather_records(records, world: int = 1, group=None):
    """All ranks' records, sorted by clip index (one collective; the identity with one rank)."""
    if world > 1:
        parts = [None] * world
        torch.distributed.all_gather_object(parts, list(records), group=group)
        records = [r for part in parts for r in part]
    return sorted(records, key=lambda r: r["index"])


def summarize(records, targeted: bool = False):
    keys = SUMMARY_FIELDS + ((TARGET_FIELD,) if targeted else ())
    n = len(records)
    out = {k: (sum(float(r[k]) for r in records) / n if n else float("nan")) for k in keys} | {"clips": n}
    if records and "found" in records[0]:          # --bound_search shrink: the share of clips that fell, the mean scale they fell at
        hit = [r for r in records if r["found"]]
        out["success_rate"] = len(hit) / n
        out["mean_bound_scale"] = sum(float(r["bound_scale"]) for r in hit) / len(hit) if hit else float("nan")
    return out


def results_dict(records, args):
    targeted = args.attack_mode == "targeted"
    return {"norm_type": str(args.norm_type), "attack_mode": args.attack_mode, "optimizer_type": args.optimizer_type,
            "split": args.split, "pgd_steps": int(args.pgd_steps), "clips": list(records),
            "summary": summarize(records, targeted)}


def write_results(path, records, args):
    with open(path, "w") as f:
        json.dump(results_dict(records, args), f, indent=2)


def _wer(pred, ref):
    e, w = loss_helpers.wer_counts([pred], [ref])
    return e / max(w, 1)


def _device_wers(args, processor, logits, texts, frames=None, blank=0):
    """Per-clip WER of ``logits`` against ``texts`` from the on-device counters (--device_wer): one (B, 3) readback.  None when
    the device route does not apply (flag off, multi-character vocabulary, a reference over the row cap): host path."""
    from .training_utils.train import device_wer_canon, log_host_route
    canon = device_wer_canon(args, processor, None, "attack_clips")
    if canon is None:
        return None
    refs = loss_helpers.encode_refs(texts)
    if refs is None:
        log_host_route("attack_clips", f"a reference needs more than {loss_helpers.R_CAP} entries")
        return None
    return [e / max(w, 1) for e, w, _ in loss_helpers.wer_counts_device(logits, refs, canon, frames=frames, blank=blank).cpu().tolist()]


def search_route(args, processor, texts):
    """(SearchConfig, canon table, the step's reference rows) of a batch under --bound_search shrink; the references are the target
    transcript in targeted mode.  Raises the table's refusal when the device WER route is not available."""
    cfg = modes.SearchConfig.of(args)
    m = modes.check(modes.Modes.of(args), modes.SEARCH_FLAGS, modes.Ctx(search=cfg))
    judged = [" ".join([args.target] * args.target_reps)] * len(texts) if cfg.targeted else texts
    canon = loss_helpers.canon_table(processor)
    refs = loss_helpers.encode_refs(judged) if canon is not None else None
    why = ("the vocabulary is not one character per token" if canon is None else
           f"a reference needs more than {loss_helpers.R_CAP} entries" if refs is None else None)
    modes.check(m, ("search_route",), modes.Ctx(search=cfg, wer_why=why))
    return cfg, canon, refs


def attack_batch(model, processor, args, x, texts, idx, interp, spl_thresh, stepper=None, lengths=None):
    """Attack one batch of clips (x (B, L) on the device) and return (records, delta, adversarial waveforms).  ``lengths``
    (--clip_lengths true): the clips' true sample counts — the model masks the padding, delta_b[len_b:] stays zero, and the
    record's norms and SNR are those of delta_b[:len_b] against x_b[:len_b].  With --bound_search shrink the delta returned,
    scored and composed is the REPORTED one: ``best_b`` of a clip that fell, the last iterate of the others."""
    B, L = x.shape
    search = None
    if modes.Modes.of(args).search_on:       # refusals first: before any launch of the batch
        search, canon, search_refs = search_route(args, processor, texts)
    labels = loss_helpers.make_labels(texts, processor, args, B)
    delta = torch.from_numpy(init_rows(L, idx, int(args.seed))).to(x.device)
    frames, blank = None, int(model.arch.pad_token_id)
    if lengths is not None:
        lengths = model.check_lengths(lengths, B)
        model.set_lengths(lengths)
        frames = model.frame_counts(B)
    elif model.lengths_on:
        model.set_lengths(None)
    project_rows(delta, x, args, interp, spl_thresh, lengths)             # build.py:301-304, per clip
    skw = {} if search is None else dict(device_wer=True, canon=canon, search=search)      # the search runs on the device WER route
    if args.optimizer_type == "adam":
        optimizer = torch.optim.Adam([delta], lr=args.lr)
        stepper = ClipStepper(model, args, L, interp, spl_thresh, optimizer=optimizer, **skw)
    elif stepper is None:
        stepper = ClipStepper(model, args, L, interp, spl_thresh, **skw)
    if search is None:
        for _ in range(int(args.pgd_steps)):
            stepper.step(delta.data, x, labels, want_logits=False)          # reads the model's length buffer, set above
        delta = delta.detach()
    else:
        stepper.set_refs(search_refs)
        stepper.search_reset(B)
        stepper.stats_log.cursor.zero_()                                    # nobody reads the per-step log here: keep it from filling
        step_logits = torch.empty(B, model.frames, model.arch.vocab_size, dtype=torch.float32, device=x.device)
        for _ in range(int(args.pgd_steps)):
            stepper.step(delta.data, x, labels, logits_out=step_logits)
        found_step = stepper.best_step[:B].clone()
        hit = found_step >= 0
        delta = torch.where(hit[:, None], stepper.best[:B], delta.detach())
        bound_scale = torch.where(hit, stepper.best_scale[:B], stepper.scale[:B]).cpu()
        last_scale, found_step = stepper.scale[:B].cpu(), found_step.cpu()
    clean_out = model.forward(x, None, labels)
    if search is None:
        adv_out = model.forward(x, delta, labels, clamp=True)
    else:       # ``found`` came from the step's own forward pass: score the reported delta through the very call the step makes
        adv_out = model.fwd_bwd(x, delta, labels, stepper.direction, want_grad=False, want_logits=True)
    clean_nll = clip_nll(model, clean_out["logits"], labels, frames).cpu()
    adv_nll = clip_nll(model, adv_out["logits"], labels, frames).cpu()
    refs = loss_helpers.clean_transcripts(texts)
    target = loss_helpers.clean_transcripts([" ".join([args.target] * args.target_reps)])[0]
    targeted = args.attack_mode == "targeted"
    dw = lambda logits, refs_: _device_wers(args, processor, logits, refs_, frames, blank)
    clean_w, adv_w = dw(clean_out["logits"], texts), dw(adv_out["logits"], texts)
    target_w = dw(adv_out["logits"], [target] * B) if targeted else None
    if clean_w is None or adv_w is None or (targeted and target_w is None):
        clean_pred, _ = loss_helpers.wer_texts(clean_out["logits"], texts, processor, frames, blank)
        adv_pred, _ = loss_helpers.wer_texts(adv_out["logits"], texts, processor, frames, blank)
        clean_w = [_wer(clean_pred[b], refs[b].lower()) for b in range(B)]
        adv_w = [_wer(adv_pred[b], refs[b].lower()) for b in range(B)]
        target_w = [_wer(adv_pred[b], target.lower()) for b in range(B)] if targeted else None
    dm, xm = delta, x
    if lengths is not None:          # the norms and the SNR of delta_b[:len_b] against x_b[:len_b]
        keep = torch.arange(L, device=x.device)[None, :] < lengths.to(x.device)[:, None]
        dm, xm = delta * keep, x * keep
    l2 = dm.norm(dim=1).cpu()
    linf = dm.abs().amax(dim=1).cpu()
    sig = xm.double().pow(2).sum(dim=1).cpu()
    noise = dm.double().pow(2).sum(dim=1).cpu()
    mloss = masking_loss(delta, x, args)[0].cpu() if modes.Modes.of(args).alpha > 0 else None
    records = []
    for b in range(B):
        rec = {"index": int(idx[b]), "clean_wer": clean_w[b], "adv_wer": adv_w[b],
               "clean_ctc": float(clean_nll[b]), "final_ctc": float(adv_nll[b]), "l2": float(l2[b]), "linf": float(linf[b]),
               "snr_db": float(10.0 * math.log10(float(sig[b]) / float(noise[b]))) if float(noise[b]) > 0 else float("inf")}
        if targeted:
            rec[TARGET_FIELD] = target_w[b]
        if mloss is not None:
            rec[MASK_FIELD] = float(mloss[b])
        if lengths is not None:
            rec[LENGTH_FIELD] = int(lengths[b])
        if search is not None:
            rec |= {"found": bool(found_step[b] >= 0), "found_step": int(found_step[b]), "bound_scale": float(bound_scale[b]),
                    "last_scale": float(last_scale[b])}
        records.append(rec)
    return records, delta, compose_rows(x, delta, lengths), stepper


def main(args) -> int:
    # what per-clip perturbations do not run with, and the refusals of --clip_lengths true: before any launch or collective
    lengths_mode = modes.check(modes.Modes.of(args), ("place_clips", "rir_clips", "chan_range", "chan_clips") + modes.LENGTHS).lengths_on
    modes.check(modes.Modes.of(args), modes.SEARCH_FLAGS + modes.MARGIN, modes.Ctx(search=modes.SearchConfig.of(args)))
    if not torch.cuda.is_available():
        raise SystemExit("paa_amd.attack_clips needs a GPU; there is no CPU fallback")
    if not str(args.device).startswith("cuda"):
        args.device = "cuda"
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    build.start_process_group(args, world)
    args.attack_size_string = build.attack_size_string(args)
    root = getattr(args, "logs_dir", None) or os.path.join(os.getcwd(), "logs")
    args.save_dir = os.path.join(root, args.attack_mode, args.dataset,
                                 f"clips_{args.norm_type}_{args.attack_size_string}{build.masking_loss_suffix(args)}_"
                                 f"{args.attack_mode}_{args.optimizer_type}")
    os.makedirs(args.save_dir, exist_ok=True)
    interp = iso.build_weight_interpolator()
    spl_thresh = build.init_phon_threshold_tensor(args)
    batches, length = split_batches(args, world)
    mine = clip_batches(batches, rank, world)
    model, processor = build.load_model(args, max_batch=max([len(item[1]) for item in mine] or [1]), length=length)
    records, stepper = [], None
    n_wav = int(args.num_items_to_inspect)
    for item in mine:
        x, texts, idx = item[:3]
        lengths = item[3] if lengths_mode else None
        if lengths_mode and len(item) < 4:
            raise ValueError("--clip_lengths true needs loaders that yield (x, texts, lengths)")
        x = x.to(args.device, torch.float32).contiguous()
        recs, _, adv, stepper = attack_batch(model, processor, args, x, texts, idx, interp, spl_thresh, stepper, lengths)
        records += recs
        for b, i in enumerate(idx):
            if i < n_wav:          # with true lengths the wav holds the clip's own len_b samples
                wav = adv[b] if lengths is None else adv[b, : int(lengths[b])]
                save.save_audio(os.path.join(args.save_dir, f"adv_clip{i}.wav"), wav, sample_rate=args.sr)
        if not getattr(args, "silent", False):
            print(f"[rank {rank}] clips {idx[0]}..{idx[-1]}: mean adv WER "
                  f"{sum(r['adv_wer'] for r in recs) / len(recs):.4f}, mean final CTC {sum(r['final_ctc'] for r in recs) / len(recs):.4f}",
                  flush=True)
    records = gather_records(records, world)
    if rank == 0:
        write_results(os.path.join(args.save_dir, "clip_results.json"), records, args)
        print(json.dumps(summarize(records, args.attack_mode == "targeted")), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(create_arg_parser().parse_args()))
