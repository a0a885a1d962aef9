"""The label-free feature-distance loss, computed by libpaa_hip.so (paa_feature_cos).  Device only: there is no CPU
fallback."""
from __future__ import annotations

import torch

from .. import _lib, runtime


def feature_distance(h: torch.Tensor, ref: torch.Tensor, frames=None, grad: bool = False, grad_scale: float = 1.0):
    """The cosine distance between the rows of two hidden states: ``h`` and ``ref`` (B, T, H) float32 on the GPU, H a multiple of 4
    in [4, 4096]; ``frames`` (B) per-clip frame counts or None.  Returns (loss, dist): loss (B,) = sum_{t < T_b} dist[b][t] and
    dist (B, T) = 1 - cos(h[b][t], ref[b][t]), zeros for t >= T_b; a row whose norm is at most 1e-8 on either side has distance 1.
    With ``grad=True`` returns (loss, dist, dh): dh (B, T, H) = grad_scale * d(sum_b loss_b) / dh, zero rows for t >= T_b and
    for the degenerate rows."""
    x = runtime.as_f32_cuda(h, "h")
    r = runtime.as_f32_cuda(ref, "ref")
    if x.dim() != 3 or tuple(r.shape) != tuple(x.shape):
        raise ValueError(f"h and ref must both be (B, T, H), got {tuple(x.shape)} and {tuple(r.shape)}")
    if r.device != x.device:
        raise RuntimeError(f"ref lives on {r.device}, h on {x.device}")
    B, T, H = x.shape
    fr = None
    if frames is not None:
        fr = torch.as_tensor(frames).to(device=x.device, dtype=torch.int32).contiguous()
        if fr.dim() != 1 or fr.numel() != B:
            raise ValueError(f"frames must hold {B} integers, got shape {tuple(fr.shape)}")
    L = _lib.lib()
    # the work buffer starts 256-byte aligned (torch's allocator), which the entry's 16-byte rule needs
    work = torch.empty(max(int(L.paa_feature_cos_work_floats(B, T)), 1), dtype=torch.float32, device=x.device)
    loss = torch.empty(B, dtype=torch.float32, device=x.device)
    dist = torch.empty(B, T, dtype=torch.float32, device=x.device)
    dh = torch.empty_like(x) if grad else None
    with torch.cuda.device(x.device):
        _lib.check(L.paa_feature_cos(_lib.ptr(x), T, _lib.ptr(r), T, _lib.ptr(fr), B, T, H, float(grad_scale), _lib.ptr(loss),
                                     _lib.ptr(dist), _lib.ptr(dh), _lib.ptr(work), _lib.stream_ptr()))
    return (loss, dist, dh) if grad else (loss, dist)
