"""Clean-signal frequency-masking threshold (the ``masking`` norm): MPEG-1 psychoacoustic model 1 on the
default frame geometry (n_fft = win_length = 1024, hop_length = 256), computed by libpaa_hip.so.  Device only: there is no
CPU fallback.  With ``args.masking_post_ms`` / ``args.masking_pre_ms`` > 0 every threshold here is spread along time (temporal
masking): the flags reach the library through the context ``runtime.get_proj`` hands out."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, runtime


def temporal_tables(args):
    """(post_db, pre_db): the float32 decrement tables of temporal masking for ``args.masking_post_ms`` /
    ``args.masking_pre_ms`` at ``args.hop_length`` / ``args.sr``; a flag that is 0 or missing gives an empty table.  A time of P ms
    lets a frame's threshold fall by 60 dB over P ms: w[j] = j 60 hop 1000 / (P sr) dB at lag j, for the lags under 96 dB."""
    if not getattr(args, "masking_post_ms", 0.0) and not getattr(args, "masking_pre_ms", 0.0):          # off: nothing to validate
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    from ..training_utils import modes
    m = modes.check(modes.Modes.of(args), ("mask_time_range",))
    tab = lambda ms: np.array([modes.mask_time_decrement(j, ms, m.hop, m.sr) for j in range(1, modes.mask_time_lags(ms, m.hop, m.sr) + 1)]
                              if ms > 0 else [], dtype=np.float64).astype(np.float32)
    return tab(m.post_ms), tab(m.pre_ms)


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


def _alpha_dev(alpha, B, dev):
    """Per-clip weights as a float32 (B) device tensor.  A host array is validated (finite, >= 0); a device tensor is taken as it
    is."""
    if isinstance(alpha, torch.Tensor) and alpha.is_cuda:
        if alpha.dtype != torch.float32 or alpha.dim() != 1 or alpha.numel() != B or not alpha.is_contiguous():
            raise ValueError(f"alpha must be a contiguous float32 tensor of {B} elements, got {alpha.dtype} {tuple(alpha.shape)}")
        return alpha.to(dev)
    a = np.asarray(alpha.cpu() if isinstance(alpha, torch.Tensor) else alpha, dtype=np.float64).reshape(-1)
    if a.size != B:
        raise ValueError(f"alpha must hold one value per clip ({B}), got {a.size}")
    if not (np.isfinite(a).all() and (a >= 0).all()):
        raise ValueError(f"every alpha must be finite and >= 0, got {a.tolist()}")
    return torch.from_numpy(a.astype(np.float32)).to(dev)


def masking_loss(delta: torch.Tensor, clean: torch.Tensor, args, grad: bool = False, alpha=None):
    """The masking-threshold loss term of ``delta`` against the clean clips ``clean`` (B, L):
    l_b = 1 / (T F) sum_{t,k} max(c_b |STFT(delta)|^2 - 10^((theta_b + masking_margin_db) / 10), 0).  ``delta`` is (1, L) or
    (L,) (the one row against every clip) or (B, L) (row b against clip b).  Returns (loss_rows (B,), grad or None): with
    ``grad=True`` the gradient of sum_b l_b itself, shaped like ``delta`` (alpha = 1, positive, not subtracted).  ``alpha``: a (B,)
    host array or device tensor of per-clip weights, for a (B, L) ``delta`` only (paa_masking_loss_rows): gradient
    row b is then alpha_b grad l_b; the losses stay unweighted."""
    x = runtime.as_f32_cuda(clean, "clean_audio")
    d = runtime.as_f32_cuda(delta, "delta")
    if x.dim() == 1:
        x = x[None]
    d2 = d[None] if d.dim() == 1 else d
    if x.dim() != 2 or d2.dim() != 2 or d2.shape[1] != x.shape[1] or d2.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"delta {tuple(d.shape)} must be (1, L) or (B, L) for clean_audio {tuple(x.shape)}")
    B, L = x.shape
    pr = runtime.get_proj(args, x.device, B, L)
    rows = torch.empty(B, dtype=torch.float32, device=x.device)
    g = torch.zeros_like(d2) if grad else None
    if alpha is not None:
        if d2.shape[0] != B:
            raise ValueError(f"per-clip alpha needs one perturbation row per clip: delta {tuple(d.shape)}, clean_audio {tuple(x.shape)}")
        al = _alpha_dev(alpha, B, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().paa_masking_loss_rows(pr.h, runtime.params_of(args, "masking"), _lib.ptr(d2), B, _lib.ptr(x), B, L,
                                                        _lib.ptr(al), B, _lib.ptr(g), _lib.ptr(rows), None, None, _lib.stream_ptr()))
        return rows, None if g is None else g.neg_().view_as(d)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().paa_masking_loss(pr.h, runtime.params_of(args, "masking"), _lib.ptr(d2), d2.shape[0], _lib.ptr(x), B, L,
                                               None, _lib.ptr(g), _lib.ptr(rows), None, None, _lib.stream_ptr()))
    if g is not None:
        g = g.neg_().view_as(d)
    return rows, g
