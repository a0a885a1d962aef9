"""Label generation, loss interface and WER bookkeeping around the HIP model — call surface of the
reference's ``src/core/loss_helpers.py``.  The tokenizer / greedy decoder / WER are small host-side
string routines (the reference delegates them to HF's ``Wav2Vec2Processor`` and ``jiwer``); when an
HF processor object is passed it is used as-is, otherwise the built-in 32-token character vocabulary
of the 960h checkpoints is used."""
from __future__ import annotations

import re

import torch

# SURVEY A.3 — vocabulary of facebook/wav2vec2-*-960h* (recalled; confirm against a local vocab.json).
VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M",
         "W", "C", "F", "G", "Y", "P", "B", "V", "K", "'", "X", "J", "Q", "Z"]
_TOK2ID = {t: i for i, t in enumerate(VOCAB)}
PAD_ID, UNK_ID = 0, 3


def clean_transcripts(texts):
    """loss_helpers.py:7-9."""
    return [re.sub(r"\s+", " ", t.replace("<unk>", "").lower()).strip() for t in texts]


def tokenize(text: str):
    """Character CTC tokenizer with do_lower_case=False: ' ' -> '|', unknown characters -> <unk>."""
    return [_TOK2ID.get(ch, UNK_ID) for ch in text.replace(" ", "|")]


def make_labels(target_texts, processor, args, batch_size: int) -> torch.Tensor:
    """loss_helpers.py:13-20 -> (B, S_max) int64 on the CPU with -100 padding."""
    if args.attack_mode == "targeted":
        target_texts = [" ".join([args.target] * args.target_reps)] * batch_size
    texts = clean_transcripts(target_texts)
    if processor is not None:
        labels = processor(text=texts, return_tensors="pt", padding=True).input_ids
        labels[labels == processor.tokenizer.pad_token_id] = -100
        return labels
    ids = [tokenize(t) for t in texts]
    smax = max(1, max(len(i) for i in ids))
    labels = torch.zeros(len(ids), smax, dtype=torch.long)
    for r, i in enumerate(ids):
        if i:
            labels[r, :len(i)] = torch.tensor(i, dtype=torch.long)
    labels[labels == PAD_ID] = -100
    return labels


def get_loss_for_training(model, data, target_texts, processor, args):
    """loss_helpers.py:12-23: ``data`` is the already composed (perturbed) batch; returns (loss, logits)
    with HF's ctc_loss_reduction='sum'.  Forward only — the PGD step gets its gradient from
    ``training_utils.pgd.PgdStepper`` in the same launch sequence."""
    labels = make_labels(target_texts, processor, args, len(data))
    r = model.forward(data, None, labels)
    return r["loss"], r["logits"]


def get_loss(batch_waveforms, target_texts, processor, args, model):
    """loss_helpers.py:46-57 — the evaluation twin of ``get_loss_for_training`` with the reference's argument
    order ``(batch_waveforms, target_texts, processor, args, model)``; same computation."""
    return get_loss_for_training(model, batch_waveforms, target_texts, processor, args)


def get_logits(batch_waveforms, processor, args, model):
    """loss_helpers.py:34-43: the only place the reference applies the processor's feature extractor, i.e.
    ``Wav2Vec2FeatureExtractor(do_normalize=True)``: per-utterance zero mean / unit variance,
    ``(x - mean) / sqrt(var + 1e-7)`` with the population variance (HF feature_extraction_wav2vec2.py
    ``zero_mean_unit_var_norm``).  A processor object, when given, is used as is (host round trip, as the
    reference does); otherwise the same normalisation runs on the device."""
    if processor is not None:
        inputs = processor(batch_waveforms.cpu().tolist(), sampling_rate=args.sr, return_tensors="pt", padding=True)
        x = inputs.input_values.to(model.device, torch.float32)
    else:
        x = batch_waveforms.to(model.device, torch.float32)
        x = (x - x.mean(dim=-1, keepdim=True)) / torch.sqrt(x.var(dim=-1, keepdim=True, unbiased=False) + 1e-7)
    return model.forward(x.contiguous(), None, None)["logits"]


def _argmax_launch(x, ids, frames=None, blank=0):
    """paa_argmax_ids on x (..., V) -> ids, or paa_argmax_ids_len on x (B, T, V) with ``frames`` (B) int32 on the device: the
    frames t >= frames[b] of clip b get the id ``blank`` (true clip lengths)."""
    from .. import _lib
    with torch.cuda.device(x.device):
        if frames is None:
            _lib.check(_lib.lib().paa_argmax_ids(_lib.ptr(x), ids.numel(), x.shape[-1], _lib.ptr(ids), _lib.stream_ptr()))
            return
        if x.dim() != 3 or frames.dtype != torch.int32 or frames.device != x.device or frames.numel() < x.shape[0]:
            raise ValueError(f"frames must be int32 ({x.shape[0]},) on the device of (B, T, V) logits")
        _lib.check(_lib.lib().paa_argmax_ids_len(_lib.ptr(x), x.shape[0], x.shape[1], x.shape[2], _lib.ptr(frames), int(blank),
                                                 _lib.ptr(ids), _lib.stream_ptr()))


def argmax_ids(logits: torch.Tensor, frames=None, blank=0) -> torch.Tensor:
    """``torch.argmax(logits, dim=-1)`` (loss_helpers.py:26,61) through the C ABI: (..., V) f32 cuda -> (...) int16.  With
    ``frames`` (per-clip frame counts), frames beyond a clip's end decode as ``blank``."""
    from .. import runtime
    x = runtime.as_f32_cuda(logits, "logits")
    ids = torch.empty(x.shape[:-1], dtype=torch.int16, device=x.device)
    _argmax_launch(x, ids, frames, blank)
    return ids


def greedy_decode_ids(pred_ids) -> list:
    """ids -> text as ``Wav2Vec2CTCTokenizer.batch_decode(skip_special_tokens=True)`` of transformers 5.15.0
    does it (pinned by tests/golden/labels.json): special ids dropped first, repeats collapsed after."""
    out = []
    for row in pred_ids:
        toks, prev = [], None
        for i in row:
            if i <= UNK_ID:
                continue
            if i != prev:
                toks.append(i)
            prev = i
        out.append("".join(" " if VOCAB[i] == "|" else VOCAB[i] for i in toks).strip())
    return out


def _edit_distance(a, b) -> int:
    d = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(b) + 1):
            cur = min(d[j] + 1, d[j - 1] + 1, prev + (a[i - 1] != b[j - 1]))
            prev, d[j] = d[j], cur
    return d[len(b)]


def wer_counts(pred_texts, ref_texts):
    """(word errors, reference words) — corpus-level WER = errors / words, jiwer's definition."""
    errs = sum(_edit_distance(r.split(), p.split()) for p, r in zip(pred_texts, ref_texts))
    return errs, sum(len(r.split()) for r in ref_texts)


def wer_texts(logits, target_texts, processor, frames=None, blank=0):
    """The two string lists loss_helpers.py:26-30 hands to the WER metric: greedy CTC decode of ``logits`` and the cleaned
    references, both lower-cased.  ``frames`` / ``blank`` as ``argmax_ids``."""
    pred_ids = argmax_ids(logits, frames, blank)
    if processor is not None:
        pred_texts = processor.batch_decode(pred_ids.long().cpu(), skip_special_tokens=True)
    else:
        pred_texts = greedy_decode_ids(pred_ids.tolist())
    return [p.strip().lower() for p in pred_texts], [t.lower() for t in clean_transcripts(target_texts)]


def compute_wer(logits, target_texts, processor, wer_metric, frames=None, blank=0):
    """loss_helpers.py:25-32."""
    pred_texts, ref_texts = wer_texts(logits, target_texts, processor, frames, blank)
    if wer_metric is not None:
        return wer_metric.compute(predictions=pred_texts, references=ref_texts)
    e, w = wer_counts(pred_texts, ref_texts)
    return e / max(w, 1)


def decode(logits, processor):
    """loss_helpers.py:60-62."""
    pred_ids = argmax_ids(logits)
    if processor is not None:
        return processor.batch_decode(pred_ids.long().cpu())
    return greedy_decode_ids(pred_ids.tolist())


# ---- on-device WER counters (paa_wer_counts) --------------------------------------------------------
R_CAP = 1024          # reference entries per clip (code points + one terminator per word): the 450-character labels of the 30 s
                      # configuration need at most 451


def canon_table(processor=None):
    """canon[V] int32 (CPU) for ``paa_wer_counts``: -1 = drop (special token), 0 = word delimiter, > 0 = the code point of the
    token's lower-cased character — what ``greedy_decode_ids`` / ``processor.batch_decode(skip_special_tokens=True)`` followed by
    ``.lower()`` make of each id.  ``processor=None``: the built-in ``VOCAB``.  Returns None when a non-special token is not a
    single character or its lower-case form is not a single code point (BPE vocabularies, 'İ'), or when lower-casing depends
    on the neighbours ('Σ'): callers then keep the host path."""
    if processor is None:
        vocab, special, delim = {t: i for i, t in enumerate(VOCAB)}, set(range(UNK_ID + 1)), "|"
    else:
        tok = getattr(processor, "tokenizer", processor)
        try:
            vocab = dict(tok.get_vocab())
            special = {int(i) for i in tok.all_special_ids}
            delim = getattr(tok, "word_delimiter_token", None)
        except Exception:       # noqa: BLE001  (not a tokenizer this table can describe)
            return None
    if not vocab or min(vocab.values()) < 0 or max(vocab.values()) > 32766:
        return None
    canon = torch.full((max(vocab.values()) + 1,), -1, dtype=torch.int32)
    for t, i in vocab.items():
        if t == delim:          # listed among the special tokens by transformers 5, yet decoded to the word boundary
            canon[i] = 0
            continue
        if i in special:
            continue
        if len(t) == 1 and t.isspace():
            canon[i] = 0
            continue
        if len(t) != 1 or t == "\u03a3" or len(t.lower()) != 1:
            return None
        canon[i] = ord(t.lower())
    return canon


def encode_refs(target_texts, r_cap: int = None):
    """Pinned int32 (B, r_cap) reference rows of ``paa_wer_counts``: the words of ``clean_transcripts(...).lower().split()`` —
    the very call ``wer_texts`` + ``wer_counts`` make, so word boundaries agree by construction — as code points, each word
    terminated by 0, the row padded with -1 (``r_cap`` defaults to ``R_CAP``).  None when a row does not fit."""
    r_cap = R_CAP if r_cap is None else r_cap
    rows = []
    for t in clean_transcripts(target_texts):
        row = []
        for w in t.lower().split():
            row.extend(ord(ch) for ch in w)
            row.append(0)
        if len(row) > int(r_cap):
            return None
        rows.append(row)
    out = torch.full((len(rows), int(r_cap)), -1, dtype=torch.int32)
    for r, row in enumerate(rows):
        if row:
            out[r, :len(row)] = torch.tensor(row, dtype=torch.int32)
    return out.pin_memory() if torch.cuda.is_available() else out


def wer_counts_device(logits_or_ids, refs, canon, out=None, sums=None, ids_out=None, frames=None, blank=0):
    """Per-clip (errors, reference words, hypothesis words) as an int32 (B, 3) device tensor, with no host round trip:
    ``paa_argmax_ids`` (when given (B, T, V) float logits; int16 (B, T) ids are used as they are) then ``paa_wer_counts``.
    ``refs`` (B, r_cap) int32 and ``canon`` (V) int32 live on the device of the logits (a CPU tensor is copied there).
    ``out`` / ``sums`` (2 floats: sum of errors, sum of reference words) / ``ids_out`` are caller-owned buffers: with all of them
    given the call allocates nothing and is graph-capturable.  ``frames`` / ``blank`` (logits only) as ``argmax_ids``."""
    from .. import _lib, runtime
    x = logits_or_ids
    dev = x.device
    if x.dtype == torch.int16:
        if x.dim() != 2 or not x.is_cuda or not x.is_contiguous():
            raise TypeError(f"ids must be a contiguous (B, T) int16 tensor on the GPU, got {tuple(x.shape)} on {x.device}")
        ids = x
    else:
        x = runtime.as_f32_cuda(x, "logits")
        if x.dim() != 3:
            raise ValueError(f"logits must be (B, T, V), got {tuple(x.shape)}")
        ids = ids_out if ids_out is not None else torch.empty(x.shape[:2], dtype=torch.int16, device=dev)
        if ids.dtype != torch.int16 or ids.numel() != x.shape[0] * x.shape[1] or ids.device != dev:
            raise ValueError("ids_out must hold B x T int16 on the device of the logits")
        _argmax_launch(x, ids, frames, blank)
    B, T = x.shape[0], x.shape[1]
    refs = refs.to(dev, non_blocking=True)
    canon = canon.to(dev, non_blocking=True)
    for name, t in (("refs", refs), ("canon", canon)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous int32 tensor")
    if refs.dim() != 2 or refs.shape[0] != B:
        raise ValueError(f"refs must be ({B}, r_cap), got {tuple(refs.shape)}")
    if out is None:
        out = torch.empty(B, 3, dtype=torch.int32, device=dev)
    if out.dtype != torch.int32 or out.numel() != B * 3 or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous (B, 3) int32 tensor on the device of the logits")
    if sums is not None and (sums.dtype != torch.float32 or sums.numel() != 2 or sums.device != dev or not sums.is_contiguous()):
        raise ValueError("sums must hold 2 contiguous float32 on the device of the logits")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().paa_wer_counts(_lib.ptr(ids), B, T, _lib.ptr(canon), canon.numel(), _lib.ptr(refs), refs.shape[1],
                                             _lib.ptr(out), _lib.ptr(sums), _lib.stream_ptr()))
    return out
