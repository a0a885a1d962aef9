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

``--loss_type feature`` (untargeted attacks): the steps push the encoder's last hidden state of x + delta away from that
of the clean x (cosine distance per frame, no labels read).  The step's ``loss`` then holds the feature distance; the records'
``clean_ctc`` / ``final_ctc`` stay CTC and the WER scoring is unchanged.  The run directory carries ``_feature`` and the results
``"loss_type": "feature"``.

``--alpha_search qin`` (needs ``--masking_loss_alpha`` > 0, the weight every clip starts from) answers "how quiet, under
the masking threshold, can this clip's successful perturbation be?": every clip carries its own weight of the masking loss, raised
while its attack succeeds and lowered while it fails, and the record describes the successful delta with the smallest masking loss
(``alpha_found``, ``alpha_step``, ``best_masking_loss``, ``best_alpha``, ``last_alpha``).  Together with ``--bound_search shrink`` the
run has two stages (Qin et al. 2019): the bound search for ``--stage1_steps`` steps without the masking loss, then the alpha
schedule for the remaining steps, started from every clip's stage-1 delta under the bound stage 1 found.

``--eot_draws G`` (with at least one of ``--place_gain_db``, ``--rir_bank``, ``--drift_ppm``, ``--noise_snr_db``) makes the
attack robust to playback: every step hears each clip's x + delta through G draws of the playback chain and sums the gradient over
them.  Afterwards the reported delta is scored through ``--eot_eval_draws`` fixed evaluation draws (``eot_adv_wer``, ``eot_clean_wer``,
``eot_success``, ``eot_draws`` in the records, their means in the summary); the direct scores stay as they are.
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
from .training_utils import build, chain, modes, parser, save
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
# --alpha_search qin only: alpha_found (a successful delta was kept), its step (-1: none), the step's own l_b of the reported delta
# (NaN: none kept), the alpha it was optimised under (the last alpha when none was kept) and the alpha the schedule ended at
ANNEAL_FIELDS = ("alpha_found", "alpha_step", "best_masking_loss", "best_alpha", "last_alpha")
STAGE1_FIELD = "stage1_masking_loss"       # two-stage run only: l_b of the delta that entered stage 2
# --eot_draws only: the reported delta through E fixed evaluation draws of the playback chain — mean WER of x + delta, of x alone
# through the same channels, the share of draws that succeed by the bound search's criterion, and E
EOT_FIELDS = ("eot_adv_wer", "eot_clean_wer", "eot_success", "eot_draws")


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
    p.add_argument("--alpha_search", type=str, choices=["off", "qin"], default="off",
                   help="qin: every clip's masking_loss_alpha starts at --masking_loss_alpha, is multiplied by --alpha_up every "
                        "--alpha_up_every steps while its attack succeeds and by --alpha_down every --alpha_down_every steps while it "
                        "fails; the record reports the successful perturbation with the smallest masking loss")
    p.add_argument("--alpha_up", type=float, default=1.2, help="alpha search: factor on success, > 1")
    p.add_argument("--alpha_down", type=float, default=0.8, help="alpha search: factor on failure, in (0, 1)")
    p.add_argument("--alpha_up_every", type=int, default=20, help="alpha search: steps between two raises")
    p.add_argument("--alpha_down_every", type=int, default=50, help="alpha search: steps between two lowerings")
    p.add_argument("--alpha_min", type=float, default=None, help="alpha search: smallest alpha (default masking_loss_alpha / 100)")
    p.add_argument("--alpha_max", type=float, default=None, help="alpha search: largest alpha (default masking_loss_alpha * 100)")
    p.add_argument("--stage1_steps", type=int, default=None,
                   help="--bound_search shrink with --alpha_search qin: steps of the bound search before the alpha schedule takes "
                        "over (default pgd_steps // 2)")
    p.add_argument("--eot_draws", type=int, default=0,
                   help=f"G in [1, {modes.EOT_DRAWS_MAX}]: every clip's adversarial example x + delta is played through G draws of the "
                        "playback chain per step (--place_gain_db, --rir_bank, --drift_ppm, --noise_snr_db; at least one) and the "
                        "gradient is summed over the draws; 0 = off")
    p.add_argument("--eot_eval_draws", type=int, default=None,
                   help="--eot_draws: fixed evaluation draws the finished perturbation is scored through (default: eot_draws)")
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
    if records and "alpha_found" in records[0]:    # --alpha_search qin: the share of clips with a kept delta, their mean l_b
        hit = [r for r in records if r["alpha_found"]]
        out["alpha_success_rate"] = len(hit) / n
        out["mean_best_masking_loss"] = sum(float(r["best_masking_loss"]) for r in hit) / len(hit) if hit else float("nan")
    if records and "eot_draws" in records[0]:      # --eot_draws: the means of the scores through the evaluation draws
        out |= {k: sum(float(r[k]) for r in records) / n for k in EOT_FIELDS[:3]}
    return out


def eot_eval_draws(args) -> int:
    """E of --eot_eval_draws (default G); 0 with the mode off."""
    g = modes.check(modes.Modes.of(args), ("eot_range",)).eot_draws
    e = getattr(args, "eot_eval_draws", None)
    e = g if e is None else e
    if g and not (isinstance(e, int) and not isinstance(e, bool) and 1 <= e <= 4096):
        raise ValueError(f"eot_eval_draws must be an integer in [1, 4096], got {e}")
    return int(e) if g else 0


def results_dict(records, args, length=None):
    """``length``: the clip length, for the chain's keys of a run with --eot_draws."""
    targeted = args.attack_mode == "targeted"
    out = {"norm_type": str(args.norm_type), "attack_mode": args.attack_mode, "optimizer_type": args.optimizer_type,
           "split": args.split, "pgd_steps": int(args.pgd_steps)} | build.masking_time_extra(args) | build.loss_extra(args)
    if modes.Modes.of(args).eot_on:
        out |= {"eot_draws": int(args.eot_draws), "eot_eval_draws": eot_eval_draws(args), **chain.results_extra(args, length)}
    return out | {"clips": list(records), "summary": summarize(records, targeted)}


def write_results(path, records, args, length=None):
    with open(path, "w") as f:
        json.dump(results_dict(records, args, length), f, indent=2)


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


def _judged_refs(args, processor, texts, targeted):
    """(canon table, the reference rows success is judged against, why the device WER route is not available or None)."""
    judged = [" ".join([args.target] * args.target_reps)] * len(texts) if targeted else texts
    canon = loss_helpers.canon_table(processor)
    refs = loss_helpers.encode_refs(judged) if canon is not None else None
    why = ("the vocabulary is not one character per token" if canon is None else
           f"a reference needs more than {loss_helpers.R_CAP} entries" if refs is None else None)
    return canon, refs, why


def search_route(args, processor, texts):
    """(SearchConfig, canon table, the step's reference rows) of a batch under --bound_search shrink; the references are the target
    transcript in targeted mode.  Raises the table's refusal when the device WER route is not available."""
    cfg = modes.SearchConfig.of(args)
    m = modes.check(modes.Modes.of(args), modes.SEARCH_FLAGS, modes.Ctx(search=cfg))
    canon, refs, why = _judged_refs(args, processor, texts, cfg.targeted)
    modes.check(m, ("search_route",), modes.Ctx(search=cfg, wer_why=why))
    return cfg, canon, refs


def anneal_route(args, processor, texts):
    """The same for --alpha_search qin: (AnnealConfig, canon table, reference rows)."""
    ctx = modes.anneal_ctx(args)
    m = modes.check(modes.Modes.of(args), modes.ANNEAL_FLAGS, ctx)
    canon, refs, why = _judged_refs(args, processor, texts, ctx.anneal.targeted)
    modes.check(m, ("anneal_route",), ctx._replace(wer_why=why))
    return ctx.anneal, canon, refs


def _begin(stepper, x):
    """What a stepper needs once per batch before its first step: under --loss_type feature the clean batch's reference features
    (after the model's lengths are set)."""
    if stepper.modes.feature_on:
        stepper.feature_reset(x)


def _run_search(stepper, delta, x, labels, steps, refs):
    """``steps`` steps of the bound search on one batch -> (reported delta, found_step, bound_scale, last_scale), the last three on
    the host.  The reported delta is ``best_b`` of a clip that fell, the last iterate of the others."""
    B = x.shape[0]
    _begin(stepper, x)
    stepper.set_refs(refs)
    stepper.search_reset(B)
    stepper.stats_log.cursor.zero_()                                    # nobody reads the per-step log here: keep it from filling
    step_logits = torch.empty(B * max(stepper.G, 1), stepper.model.frames, stepper.model.arch.vocab_size, dtype=torch.float32, device=x.device)
    for _ in range(int(steps)):
        stepper.step(delta.data, x, labels, logits_out=step_logits)
    found_step = stepper.best_step[:B].clone()
    hit = found_step >= 0
    delta = torch.where(hit[:, None], stepper.best[:B], delta.detach())
    bound_scale = torch.where(hit, stepper.best_scale[:B], stepper.scale[:B]).cpu()
    return delta, found_step.cpu(), bound_scale, stepper.scale[:B].cpu()


def _run_anneal(stepper, delta, x, labels, steps, refs):
    """``steps`` steps of the alpha schedule on one batch -> (last iterate, best rows, and on the host: alpha_step, best_loss,
    best_alpha, last_alpha, l_b of the delta that entered)."""
    B = x.shape[0]
    _begin(stepper, x)
    stepper.set_refs(refs)
    stepper.anneal_reset(B)
    stepper.stats_log.cursor.zero_()
    step_logits = torch.empty(B, stepper.model.frames, stepper.model.arch.vocab_size, dtype=torch.float32, device=x.device)
    entered = None
    for i in range(int(steps)):
        stepper.step(delta.data, x, labels, logits_out=step_logits)
        if i == 0:
            entered = stepper.mask_rows[:B].clone()
    return (delta.detach(), stepper.best[:B].clone(), stepper.best_step[:B].cpu(), stepper.best_loss[:B].cpu(),
            stepper.best_alpha[:B].cpu(), stepper.alpha_rows[:B].cpu(), entered.cpu())


def eot_scores(model, processor, args, stepper, x, delta, texts):
    """The reported ``delta`` (B, L) of a batch through E fixed evaluation draws of the playback chain (``stepper.eval_rows``: the
    evaluation stream at steps 0, 1, ..., G draws per pass) -> {field of EOT_FIELDS: one value per clip}.  The clean clips go
    through the same channels, noise included.  A draw succeeds by the bound search's criterion: WER against the clip's own
    transcript >= --search_success_wer (rounded to thousandths), or in targeted mode the target transcript exactly."""
    B, G, E = x.shape[0], stepper.G, eot_eval_draws(args)
    targeted = args.attack_mode == "targeted"
    milli, blank = modes._wer_milli(args), int(model.arch.pad_token_id)
    rep = lambda seq: [t for t in seq for _ in range(G)]
    row_texts = rep(texts)
    judged = [" ".join([args.target] * args.target_reps)] * (B * G) if targeted else row_texts
    labels = loss_helpers.make_labels(row_texts, processor, args, B * G)
    zero, none = stepper.zero_rows[: B * G], torch.zeros_like(delta)
    adv, cln, hits = [[] for _ in range(B)], [[] for _ in range(B)], [0] * B

    def decode(p):
        """Greedy transcripts of the rows the microphone hears (clipped, as in the step)."""
        return loss_helpers.wer_texts(model.forward(zero, p, labels, clamp=True)["logits"], row_texts, processor, None, blank)[0]

    def counts(pred, refs):
        """Per-row (errors, reference words)."""
        return [loss_helpers.wer_counts([a], [b.lower()]) for a, b in zip(pred, loss_helpers.clean_transcripts(refs))]

    for k in range(-(-E // G)):
        keep = min(G, E - k * G)                     # the last pass may hold more draws than are still wanted
        pred = decode(stepper.eval_rows(delta, x, k))
        heard = counts(pred, row_texts)
        judge = counts(pred, judged) if targeted else heard
        clean = counts(decode(stepper.eval_rows(none, x, k)), row_texts)
        for b in range(B):
            for g in range(keep):
                r = b * G + g
                adv[b].append(heard[r][0] / max(heard[r][1], 1))
                cln[b].append(clean[r][0] / max(clean[r][1], 1))
                e, w = judge[r]
                hits[b] += int(w > 0 and (e == 0 if targeted else e * 1000 >= milli * w))
    return {"eot_adv_wer": [sum(v) / E for v in adv], "eot_clean_wer": [sum(v) / E for v in cln],
            "eot_success": [h / E for h in hits], "eot_draws": [E] * B}


def attack_batch(model, processor, args, x, texts, idx, interp, spl_thresh, stepper=None, lengths=None):
    """Attack one batch of clips (x (B, L) on the device) and return (records, delta, adversarial waveforms).  ``lengths``
    (--clip_lengths true): the clips' true sample counts — the model masks the padding, delta_b[len_b:] stays zero, and the
    record's norms and SNR are those of delta_b[:len_b] against x_b[:len_b].  With --bound_search shrink the delta returned,
    scored and composed is the REPORTED one: ``best_b`` of a clip that fell, the last iterate of the others."""
    B, L = x.shape
    search = anneal = None
    if modes.Modes.of(args).search_on:       # refusals first: before any launch of the batch
        search, canon, search_refs = search_route(args, processor, texts)
    if modes.Modes.of(args).anneal_on:
        anneal, canon, search_refs = anneal_route(args, processor, texts)
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
    steps, stage1 = int(args.pgd_steps), 0
    G = modes.Modes.of(args).eot_draws if modes.Modes.of(args).eot_on else 0
    if anneal is None:
        skw = {} if search is None else dict(device_wer=True, canon=canon, search=search)      # the search runs on the device WER route
        if G:
            skw["eot_draws"] = G
        if args.optimizer_type == "adam":
            optimizer = torch.optim.Adam([delta], lr=args.lr)
            stepper = ClipStepper(model, args, L, interp, spl_thresh, optimizer=optimizer, **skw)
        elif stepper is None:
            stepper = ClipStepper(model, args, L, interp, spl_thresh, **skw)
        if G:       # a clip's draws depend on (seed, its global index, draw, step) alone: row ids from the index, steps from 0
            if list(idx) != list(range(int(idx[0]), int(idx[0]) + B)):
                raise ValueError(f"--eot_draws needs a shard of contiguous clip indices, got {list(idx)}")
            stepper.set_eot_clip(int(idx[0]))
            stepper.set_eot_step(0)
        if search is None:
            _begin(stepper, x)
            for _ in range(steps):
                stepper.step(delta.data, x, labels, want_logits=False)          # reads the model's length buffer, set above
            delta = delta.detach()
        else:
            delta, found_step, bound_scale, last_scale = _run_search(stepper, delta, x, labels, steps, search_refs)
    else:
        adam = args.optimizer_type == "adam"
        akw = dict(device_wer=True, canon=canon, anneal=anneal)
        if search is not None:       # stage 1: the bound search as it runs alone, the masking loss off (steppers of a batch: not reused)
            stage1 = modes.stage1_of(getattr(args, "stage1_steps", None), steps)
            args1 = copy.copy(args)
            args1.masking_loss_alpha = 0.0
            st1 = ClipStepper(model, args1, L, interp, spl_thresh, optimizer=torch.optim.Adam([delta], lr=args.lr) if adam else None,
                              device_wer=True, canon=canon, search=search)
            delta, found_step, bound_scale, last_scale = _run_search(st1, delta, x, labels, stage1, search_refs)
            entered_delta = delta.clone()                        # stage 2 starts from the stage-1 reported delta ...
            akw["bound_scale"] = bound_scale.to(x.device)        # ... under the bound that delta satisfies
            stepper = None
        if adam or stepper is None or stepper.anneal != anneal:
            stepper = ClipStepper(model, args, L, interp, spl_thresh, optimizer=torch.optim.Adam([delta], lr=args.lr) if adam else None,
                                  **akw)
        last, best, alpha_step, best_loss, best_alpha, last_alpha, entered_loss = _run_anneal(stepper, delta, x, labels, steps - stage1,
                                                                                             search_refs)
        kept = (alpha_step >= 0).to(x.device)
        if search is not None:       # a clip stage 2 never kept keeps its stage-1 best, where there is one
            last = torch.where((found_step >= 0).to(x.device)[:, None], entered_delta, last)
        delta = torch.where(kept[:, None], best, last)
    clean_out = model.forward(x, None, labels)
    if search is None and anneal is None:
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
    eot = eot_scores(model, processor, args, stepper, x, delta, texts) if G else None
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
        if anneal is not None:
            ok = bool(alpha_step[b] >= 0)
            rec |= {"alpha_found": ok, "alpha_step": int(alpha_step[b]), "best_masking_loss": float(best_loss[b]) if ok else float("nan"),
                    "best_alpha": float(best_alpha[b] if ok else last_alpha[b]), "last_alpha": float(last_alpha[b])}
            if search is not None:
                rec[STAGE1_FIELD] = float(entered_loss[b])
        if eot is not None:
            rec |= {k: eot[k][b] for k in EOT_FIELDS}
        records.append(rec)
    return records, delta, compose_rows(x, delta, lengths), stepper


def main(args) -> int:
    # what per-clip perturbations do not run with, and the refusals of --clip_lengths true: before any launch or collective
    # --eot_draws lifts the three "per-clip" refusals and puts its own rules, then the links' own flag checks, in their place
    eot = modes.check(modes.Modes.of(args), ("eot_range",)).eot_on
    per_clip = ("chan_range",) + modes.EOT if eot else ("place_clips", "rir_clips", "chan_range", "chan_clips")
    lengths_mode = modes.check(modes.Modes.of(args), per_clip + modes.LENGTHS).lengths_on
    if eot:
        chain.check_flags(args)
        eot_eval_draws(args)
    modes.check(modes.Modes.of(args), modes.SEARCH_FLAGS + modes.MARGIN + modes.FEATURE, modes.Ctx(search=modes.SearchConfig.of(args)))
    modes.check(modes.Modes.of(args), modes.ANNEAL_FLAGS, modes.anneal_ctx(args))
    modes.check(modes.Modes.of(args), modes.MASK_TIME)
    if not torch.cuda.is_available():
        raise SystemExit("paa_amd.attack_clips needs a GPU; there is no CPU fallback")
    if not str(args.device).startswith("cuda"):
        args.device = "cuda"
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    build.start_process_group(args, world)
    args.attack_size_string = build.attack_size_string(args)
    root = getattr(args, "logs_dir", None) or os.path.join(os.getcwd(), "logs")
    args.save_dir = os.path.join(root, args.attack_mode, args.dataset,
                                 f"clips_{args.norm_type}_{args.attack_size_string}{build.masking_loss_suffix(args)}{build.masking_time_suffix(args)}{build.loss_suffix(args)}"
                                 f"{chain.suffix(args) + f'_eot{int(args.eot_draws)}' if eot else ''}_"
                                 f"{args.attack_mode}_{args.optimizer_type}")
    os.makedirs(args.save_dir, exist_ok=True)
    interp = iso.build_weight_interpolator()
    spl_thresh = build.init_phon_threshold_tensor(args)
    batches, length = split_batches(args, world)
    mine = clip_batches(batches, rank, world)
    rows_per_clip = int(args.eot_draws) if eot else 1          # the model hears every clip through that many draws
    model, processor = build.load_model(args, max_batch=max([len(item[1]) for item in mine] or [1]) * rows_per_clip, length=length)
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
        write_results(os.path.join(args.save_dir, "clip_results.json"), records, args, length)
        print(json.dumps(summarize(records, args.attack_mode == "targeted")), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(create_arg_parser().parse_args()))
