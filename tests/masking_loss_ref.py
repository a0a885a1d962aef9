"""float64 numpy restatement of the masking-threshold loss term, on top of tests/masking_ref.py:

    l_b(delta) = 1 / (T F) sum_{t,k} max(c_b |S(t,k)|^2 - 10^((theta_b(t,k) + m) / 10), 0),   c_b = 10^((96 - Pmax_b) / 10)

with S = STFT(delta), the strict hinge (active iff |S|^2 > A_b^2), and the gradient of sum_b l_b as the ADJOINT of the STFT
applied to H = W S.  ``torch_loss`` is the same loss written through oracle.projections.compute_stft for autograd."""
import numpy as np
import torch

import masking_ref as MR
from oracle import projections as OP

N_FFT, HOP, F = MR.N_FFT, MR.HOP, MR.F


def hann_periodic(n=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def scale(pmax):
    return 10.0 ** ((96.0 - float(pmax)) / 10.0)


def weight(S, thetas, pmaxs, margin=0.0):
    """S (T, F) complex128 -> W (T, F) and the per-clip active masks (B, T, F)."""
    T, Fb = S.shape
    pw = np.abs(S) ** 2
    act = np.stack([pw > MR.bound(th, pm, margin) ** 2 for th, pm in zip(thetas, pmaxs)])
    c = np.array([scale(pm) for pm in pmaxs])
    return (c[:, None, None] * act).sum(0) / (T * Fb), act


def loss_rows(S, thetas, pmaxs, margin=0.0):
    """(B,) l_b."""
    pw = np.abs(S) ** 2
    with np.errstate(over="ignore"):
        return np.array([np.maximum(scale(pm) * pw - 10.0 ** ((np.asarray(th, dtype=np.float64) + margin) / 10.0), 0.0).mean()
                         for th, pm in zip(thetas, pmaxs)])


def adjoint(W, S, L):
    """Gradient of sum_b l_b with respect to delta, (L,): fold(overlap_add(w 1024 irfft(H))), H = W S, DC / Nyquist doubled."""
    H = W * S
    H[:, 0] *= 2
    H[:, -1] *= 2
    y = np.fft.irfft(H, n=N_FFT, axis=1) * N_FFT * hann_periodic(N_FFT)
    gp = np.zeros(L + N_FFT)
    for t in range(S.shape[0]):
        gp[HOP * t: HOP * t + N_FFT] += y[t]
    g = gp[N_FFT // 2: N_FFT // 2 + L].copy()
    i = np.arange(1, N_FFT // 2 + 1)
    np.add.at(g, i, gp[N_FFT // 2 - i])
    np.add.at(g, L - 1 - i, gp[N_FFT // 2 + L - 1 + i])
    return g


def grad(delta, thetas, pmaxs, margin=0.0):
    """(gradient of sum_b l_b (L,), W, S) for one perturbation row held against the given clips."""
    S = MR.stft_tf(delta)
    W, _ = weight(S, thetas, pmaxs, margin)
    return adjoint(W, S, np.asarray(delta).shape[-1]), W, S


def ambiguous(S, thetas, pmaxs, margin=0.0, tol=4e-5):
    """(B, T, F) bool: | |S| - A_b | <= tol max|S| — the hinge decision of an f32 STFT may legitimately differ there."""
    mag = np.abs(S)
    return np.stack([np.abs(mag - MR.bound(th, pm, margin)) <= tol * mag.max() for th, pm in zip(thetas, pmaxs)])


def torch_loss(delta_t, thetas, pmaxs, margin=0.0):
    """sum_b l_b of a float64 torch tensor (L,), differentiable: the loss through oracle.projections.compute_stft."""
    S = OP.compute_stft(delta_t[None], MR._args())[0].transpose(0, 1)            # (T, F)
    pw = S.real ** 2 + S.imag ** 2
    tot = 0.0
    for th, pm in zip(thetas, pmaxs):
        with np.errstate(over="ignore"):
            lim = torch.from_numpy(10.0 ** ((np.asarray(th, dtype=np.float64) + margin) / 10.0))
        tot = tot + torch.clamp(scale(pm) * pw - lim, min=0.0).mean()
    return tot
