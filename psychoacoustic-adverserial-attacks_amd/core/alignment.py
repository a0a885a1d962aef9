"""Forced alignment and the alignment-margin loss, computed by libpaa_hip.so (paa_align_margin).  Device only:
there is no CPU fallback."""
from __future__ import annotations

import torch

from .. import _lib, runtime


def _run(logits, labels, kappa, frames, blank, want_align, grad_scale=None):
    z = runtime.as_f32_cuda(logits, "logits")
    if z.dim() != 3:
        raise ValueError(f"logits must be (B, T, V), got {tuple(z.shape)}")
    B, T, V = z.shape
    lab = torch.as_tensor(labels).to(device=z.device, dtype=torch.int32).contiguous()
    if lab.dim() != 2 or lab.shape[0] != B or lab.shape[1] < 1:
        raise ValueError(f"labels must be (B, S) = ({B}, >= 1), got {tuple(lab.shape)}")
    fr = None
    if frames is not None:
        fr = torch.as_tensor(frames).to(device=z.device, dtype=torch.int32).contiguous()
        if fr.dim() != 1 or fr.numel() != B:
            raise ValueError(f"frames must hold {B} integers, got shape {tuple(fr.shape)}")
    L = _lib.lib()
    S = lab.shape[1]
    # the work buffer starts 256-byte aligned (torch's allocator), which the entry's 16-byte rule needs
    work = torch.empty(max(int(L.paa_align_margin_work_floats(B, T, V, S)), 1), dtype=torch.float32, device=z.device)
    loss = torch.empty(B, dtype=torch.float32, device=z.device)
    align = torch.empty(B, T, dtype=torch.int16, device=z.device) if want_align else None
    dl = torch.empty_like(z) if grad_scale is not None else None
    with torch.cuda.device(z.device):
        _lib.check(L.paa_align_margin(_lib.ptr(z), _lib.ptr(lab), _lib.ptr(fr), B, T, T, V, S, int(blank), float(kappa),
                                      float(grad_scale or 0.0), _lib.ptr(loss), _lib.ptr(align), _lib.ptr(dl), None, None,
                                      _lib.ptr(work), _lib.stream_ptr()))
    return loss, align, dl


def forced_alignment(logits: torch.Tensor, labels, frames=None, blank: int = 0) -> torch.Tensor:
    """The Viterbi alignment of every label row to its clip's frames: ``logits`` (B, T, V) float32 on the GPU, ``labels`` (B, S)
    integers (negatives = padding), ``frames`` (B) per-clip frame counts or None -> (B, T) int16 class ids, ``blank`` for the
    frames past a clip's end and for a label row that its frames cannot spell.  Frame t of clip b belongs to the character
    ids[b, t]: per-character timing."""
    return _run(logits, labels, 0.0, frames, blank, True)[1]


def margin_loss(logits: torch.Tensor, labels, kappa: float, frames=None, blank: int = 0, grad: bool = False):
    """The alignment-margin loss l_b = sum_t max(kappa + max_{c != pi_t} z[t][c] - z[t][pi_t], 0) over the forced alignment pi
    of the current logits -> (B,) float32, +inf for a label row that the frames cannot spell.  With ``grad=True`` returns
    (loss, dlogits): the cotangent of sum_b l_b with pi held fixed."""
    loss, _, dl = _run(logits, labels, kappa, frames, blank, False, 1.0 if grad else None)
    return (loss, dl) if grad else loss
