"""Clean-signal frequency-masking threshold (the ``masking`` norm): MPEG-1 psychoacoustic model 1 on the
default frame geometry (n_fft = win_length = 1024, hop_length = 256), computed by libpaa_hip.so.  Device only: there is no
CPU fallback."""
from __future__ import annotations

import torch

from .. import _lib, runtime


def masking_threshold(clean: torch.Tensor, args, psd: bool = False):
    """``clean`` (B, L) or (L,) float32 on the GPU -> (theta_db (B, T, F), pmax (B,)), T = 1 + L // 256, F = 513:
    theta is the global masking threshold of each frame in dB on the normalised scale P - pmax + 96 (-inf where no masker
    and no threshold in quiet reaches the bin), pmax the clip's maximum level 10 log10(|STFT|^2 + 1e-20).  With ``psd=True``
    the normalised levels P - pmax + 96 (B, T, F) are returned third."""
    x = runtime.as_f32_cuda(clean, "clean_audio")
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2:
        raise ValueError(f"clean_audio must be (B, L), got {tuple(x.shape)}")
    B, L = x.shape
    pr = runtime.get_proj(args, x.device, B, L)
    T, F = 1 + L // pr.hop, pr.F
    theta = torch.empty(B, T, F, dtype=torch.float32, device=x.device)
    pmax = torch.empty(B, dtype=torch.float32, device=x.device)
    pb = torch.empty_like(theta) if psd else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().paa_masking_threshold(pr.h, _lib.ptr(x), B, L, _lib.ptr(pb), _lib.ptr(theta), _lib.ptr(pmax),
                                                    _lib.stream_ptr()))
    return (theta, pmax, pb) if psd else (theta, pmax)
