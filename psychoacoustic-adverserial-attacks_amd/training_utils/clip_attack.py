"""Per-clip (per-utterance) attacks: one perturbation row delta_b per clip b, on the device step.

Semantics (a per-clip step on B clips is B independent universal steps at batch 1):

    x~_b = clamp(x_b + delta_b, -1, 1)      loss = sum_b CTC_b (HF reduction='sum')
    g_b  = direction * dloss / ddelta_b     (in eval mode CTC_b depends on delta_b alone)
    delta_b += lr * sign(g_b)   |   torch.optim.Adam over the (B, L) tensor
    delta_b  = perturbation_constraint(delta_b[None], x_b[None], args)   for every norm of args.norm_type, in order

With ``args.masking_loss_alpha`` = alpha > 0 clip b's objective is direction * CTC_b - alpha * l_b(delta_b):
``paa_masking_loss`` with one row per clip subtracts alpha * grad l_b from row b of the gradient right after the backward pass.

One launch sequence per step (``paa_model_fwd_bwd_rows`` -> ``paa_sign_step`` / ``paa_adam_step`` over B*L elements ->
``paa_project_rows`` per norm) and no collective: clips are independent, so ranks never exchange gradients.  The Adam
bookkeeping (optimizer.state, the pinned ring of per-step scalars, replay of a captured graph) is PgdStepper's.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, runtime, synth
from .pgd import N_STATS, RING, ST_LOSS, ST_MASK_LOSS, PgdStepper, _AdamGraph, adam_unsupported


class ClipStepper(PgdStepper):
    """The per-clip step: ``step(delta, clean, labels)`` updates ``delta`` (B, L) in place, row b from clip b alone."""

    def __init__(self, model, args, length: int, interp=None, spl_thresh=None, optimizer=None, device_wer=False, canon=None,
                 r_cap=None, log_cap=4096):
        """``device_wer`` / ``canon`` / ``r_cap`` / ``log_cap`` as PgdStepper's; ``wer_rows[:B]`` keeps the per-clip (errors,
        reference words, hypothesis words) of the last step."""
        self.model, self.args, self.L = model, args, int(length)
        self.dev = model.device
        self.norms = str(args.norm_type).split("+")
        for n in self.norms:
            if n not in _lib.NORM_IDS:
                raise ValueError(f"Unknown norm_type: {n!r}")                  # train.py:98
        self.direction = +1 if args.attack_mode == "untargeted" else -1          # train.py:124
        self.max_batch = int(model.max_batch)
        self.grad_buf = torch.zeros(self.max_batch * self.L, dtype=torch.float32, device=self.dev)
        self.grad = self.grad_buf[: self.L].view(1, self.L)
        self.stats = torch.zeros(N_STATS, dtype=torch.float32, device=self.dev)
        self.packed = None
        self.proj = runtime.get_proj(args, self.dev, self.max_batch, self.L, interp)
        if spl_thresh is not None:
            self.proj.set_spl_thresh(spl_thresh)
        self.group, self.world, self.collective, self.need_clean_stats = None, 1, False, False
        self._prm = []
        for n in self.norms:
            a = type("A", (), dict(vars(args)))()
            a.norm_type = n
            self._prm.append(runtime.params_of(a))
        self._wer_next = (0.0, 0.0)
        self.optimizer = optimizer
        if optimizer is not None:
            why = adam_unsupported(optimizer)
            if why is not None:
                raise NotImplementedError(f"the device Adam step does not implement {why}")
            self.adam_p = optimizer.param_groups[0]["params"][0]
            if self.adam_p.dim() != 2 or self.adam_p.shape[1] != self.L or self.adam_p.shape[0] > self.max_batch:
                raise ValueError(f"optimizer parameter has shape {tuple(self.adam_p.shape)}, expected (B, {self.L}) with "
                                 f"B <= {self.max_batch}")
            self.adam_scal = torch.zeros(2, dtype=torch.float32, device=self.dev)
            self.adam_grad = torch.zeros_like(self.adam_p, dtype=torch.float32, device=self.dev)
        self._ring = [torch.zeros(4, dtype=torch.float32).pin_memory() for _ in range(RING)] if optimizer is not None else None
        self._ring_ev = [None] * RING
        self._ring_i = 0
        self.mask_rows = torch.zeros(self.max_batch, dtype=torch.float32, device=self.dev)      # l_b of the last step
        self._init_masking_loss()
        self._init_device_wer(device_wer, canon, r_cap, log_cap)

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
        grad = self.grad_buf[: B * L].view(B, L)
        self.grad = grad
        out = {"grad": grad, "stats": self.stats}
        if logits_out is not None:
            out["logits"] = logits_out
        r = self.model.fwd_bwd(clean, delta, labels, self.direction, want_grad=True, want_logits=want_logits, out=out)
        if self.mask_alpha > 0:
            self._masking_loss(delta, clean, grad, self.mask_rows[:B])
            r["masking_loss"] = self.mask_rows[:B]
        if self.device_wer:
            self._wer(r["logits"], B)
        with torch.cuda.device(self.dev):
            st = _lib.stream_ptr()
            if self.optimizer is None:
                _lib.check(lib.paa_sign_step(_lib.ptr(delta), _lib.ptr(grad), float(self.args.lr), B * L, st))
            else:                       # Adam minimises -direction * loss; grad = d(direction * loss)
                w1, b2, omb2, eps = self.adam_consts()
                ast = self._adam_state()
                _lib.check(lib.paa_adam_step(_lib.ptr(delta), _lib.ptr(grad), -1.0, _lib.ptr(ast["exp_avg"]),
                                             _lib.ptr(ast["exp_avg_sq"]), _lib.ptr(self.adam_scal), w1, b2, omb2, eps,
                                             _lib.ptr(self.adam_grad), B * L, st))
            for prm in self._prm:
                _lib.check(lib.paa_project_rows(self.proj.h, prm, _lib.ptr(delta), _lib.ptr(delta), B, _lib.ptr(clean), L, st))
        if self.device_wer:
            self.stats_log.push(self.stats)
        r["loss"] = self.stats[ST_LOSS]
        r["grad"] = grad
        return r

    def step(self, delta: torch.Tensor, clean: torch.Tensor, labels: torch.Tensor, want_logits=True, logits_out=None,
             refs=None):
        """In place on ``delta`` (B, L).  Returns dict(loss: 0-d device tensor, the sum over the clips, logits, grad (B, L)).
        ``refs`` as PgdStepper.step."""
        if refs is not None:
            self.set_refs(refs)
        delta, clean = self._checked(delta, clean)
        self._check_p(delta)
        self._pre_step()
        return self._body(delta, clean, labels, want_logits, logits_out)

    def capture(self, delta, clean, labels, logits_out=None, refs=None):
        """One step on fixed buffers as ONE hipGraph (``refs`` as PgdStepper.capture).  Returns (graph, result dict); ``graph.replay()`` re-runs the step in
        place on ``delta`` with whatever ``clean`` / ``labels`` hold.  With Adam the graph is wrapped so that every replay
        first pushes the step's scalars, and the warm-up step is undone (delta, moments and step count as before the call)."""
        delta, clean = self._checked(delta, clean)
        lab = labels.to(device=self.dev, dtype=torch.int32).contiguous()
        self._alpha_captured = self.mask_alpha > 0
        saved = None
        if self.optimizer is not None:
            self._check_p(delta)
            ast = self._adam_state()
            saved = (delta.detach().clone(), ast["exp_avg"].clone(), ast["exp_avg_sq"].clone(), ast["step"].clone())
        if logits_out is None:
            logits_out = torch.empty(clean.shape[0], self.model.frames, self.model.arch.vocab_size, device=self.dev)
        self._captured_buffers = (lab, logits_out)        # the graphs hold raw pointers: keep what capture() itself created alive
        cur0 = None
        if self.device_wer:
            if refs is not None:
                self.set_refs(refs)
            cur0 = self.stats_log.cursor.clone()
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(s):                       # warm-up on the side stream, as torch's capture rules require
            self.step(delta, clean, lab, logits_out=logits_out)
        torch.cuda.current_stream(self.dev).wait_stream(s)
        if cur0 is not None:
            self.stats_log.cursor.copy_(cur0)
        if saved is not None:
            torch.cuda.synchronize(self.dev)
            delta.detach().copy_(saved[0])
            ast["exp_avg"].copy_(saved[1])
            ast["exp_avg_sq"].copy_(saved[2])
            ast["step"].copy_(saved[3])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            r = self._body(delta, clean, lab, logits_out=logits_out)
        if self.optimizer is None:
            return g, r
        return _AdamGraph(self, g), r


# ---------------------------------------------------------------------------------------------------- host helpers
def init_rows(length: int, indices, seed: int = 5) -> np.ndarray:
    """(len(indices), L) float32 standard normals: the stand-in of build.init_perturbation's ``torch.randn(1, L)`` for each
    clip, keyed by the clip's GLOBAL index (its position in the split), so that a clip's draw depends neither on the batch it
    lands in nor on the number of ranks."""
    out = np.empty((len(indices), int(length)), dtype=np.float32)
    for r, i in enumerate(indices):
        out[r] = synth.normal(synth.key_of(f"p0_clip{int(i)}", int(seed)), int(length)).astype(np.float32)
    return out


def project_rows(delta: torch.Tensor, clean: torch.Tensor, args, interp=None, spl_thresh=None) -> torch.Tensor:
    """perturbation_constraint (train.py:69-99) on every row of ``delta`` (B, L) against its own clip of ``clean`` (B, L),
    in place; the norms of ``args.norm_type`` in order."""
    delta = runtime.as_f32_cuda(delta, "delta")
    clean = runtime.as_f32_cuda(clean, "clean_audio")
    if delta.dim() != 2 or tuple(delta.shape) != tuple(clean.shape):
        raise ValueError(f"delta {tuple(delta.shape)} and clean_audio {tuple(clean.shape)} must both be (B, L)")
    B, L = delta.shape
    pr = runtime.get_proj(args, delta.device, B, L, interp)
    with torch.cuda.device(delta.device):
        for n in str(args.norm_type).split("+"):
            if n not in _lib.NORM_IDS:
                raise ValueError(f"Unknown norm_type: {n!r}")
            a = type("A", (), dict(vars(args)))()
            a.norm_type = n
            if n == "max_phon":
                pr.set_spl_thresh(spl_thresh)
            _lib.check(_lib.lib().paa_project_rows(pr.h, runtime.params_of(a), _lib.ptr(delta), _lib.ptr(delta), B,
                                                   _lib.ptr(clean), L, _lib.stream_ptr()))
    return delta


def compose_rows(clean: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """clamp(clean_b + delta_b, -1, 1) for every clip (the adversarial waveforms the entry point writes)."""
    clean = runtime.as_f32_cuda(clean, "clean_audio")
    delta = runtime.as_f32_cuda(delta, "delta")
    B, L = clean.shape
    out = torch.empty_like(clean)
    with torch.cuda.device(clean.device):
        _lib.check(_lib.lib().paa_compose_clamp_rows(_lib.ptr(clean), _lib.ptr(delta), delta.shape[0] if delta.dim() == 2 else 1,
                                                     _lib.ptr(out), B, L, _lib.stream_ptr()))
    return out


def clip_nll(model, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Per-clip CTC loss (B,) of logits (B, T, V) on the device (paa_ctc, HF reduction 'sum' per clip)."""
    lab = labels.to(device=logits.device, dtype=torch.int32).contiguous()
    B, T, V = logits.shape
    S = lab.shape[1]
    L = _lib.lib()
    work = torch.empty(int(L.paa_ctc_work_floats(B, T, V, S)), dtype=torch.float32, device=logits.device)
    nll = torch.empty(B, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(L.paa_ctc(_lib.ptr(logits.contiguous()), _lib.ptr(lab), B, T, V, S, int(model.arch.pad_token_id), 1.0,
                             _lib.ptr(nll), None, _lib.ptr(work), _lib.stream_ptr()))
    return nll
