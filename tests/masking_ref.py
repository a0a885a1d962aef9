"""float64 numpy restatement of the masking norm: the clean clip's MPEG-1 psychoacoustic model 1 threshold on
the default frame geometry and the projection that clips the perturbation's STFT to it.  STFT, iSTFT and the length rule come
from oracle.projections.  ``threshold_from_pbar`` starts from given normalised levels so that a test can feed it the device's
own P - Pmax + 96 and share every discrete decision; it also reports, per frame, the smallest gap of a decision it took."""
import numpy as np
import torch

from oracle import projections as OP

N_FFT, HOP, F = 1024, 256, 513


def bark(f):
    f = np.asarray(f, dtype=np.float64)
    return 13.0 * np.arctan(0.00076 * f) + 3.5 * np.arctan((f / 7500.0) ** 2)


def quiet(f):
    """Threshold in quiet (dB); +inf at 0 Hz."""
    fk = np.asarray(f, dtype=np.float64) / 1000.0
    with np.errstate(divide="ignore"):
        return 3.64 * fk ** -0.8 - 6.5 * np.exp(-0.6 * (fk - 3.3) ** 2) + 1e-3 * fk ** 4 - 12.0


def tables(sr):
    """z (F), quiet (F), ATH (F, nan below kA), kA, lo (F), hi (F)."""
    f = np.arange(F, dtype=np.float64) * sr / N_FFT
    z = bark(f)
    q = quiet(f)
    kA = int(np.argmax(z > 1.0))
    ath = np.where(np.arange(F) >= kA, q, np.nan)
    lo = np.empty(F, dtype=np.int64)
    hi = np.empty(F, dtype=np.int64)
    for k in range(F):
        inside = np.nonzero(np.abs(z - z[k]) < 0.5)[0]
        lo[k], hi[k] = inside[0], inside[-1]
        assert np.all(np.diff(inside) == 1)
    return z, q, ath, kA, lo, hi


def stft_tf(x):
    """(L,) -> (T, F) complex128 STFT (paa_stft's frame-major layout)."""
    s = OP.compute_stft(torch.from_numpy(np.asarray(x, dtype=np.float64)[None]), _args())
    return s[0].numpy().T


def levels(x):
    """P (T, F) = 10 log10(|X|^2 + 1e-20) and Pmax."""
    X = stft_tf(x)
    P = 10.0 * np.log10(np.abs(X) ** 2 + 1e-20)
    return P, float(P.max())


def threshold_from_pbar(pbar, sr):
    """pbar (T, F) normalised levels -> theta (T, F) dB, decision margin (T,), survivors per frame (T,), survivor mask (T, F)."""
    pb = np.asarray(pbar, dtype=np.float64)
    z, q, ath, kA, lo, hi = tables(sr)
    T = pb.shape[0]
    cand = np.zeros_like(pb, dtype=bool)
    cand[:, 1:F - 1] = (pb[:, 1:F - 1] > pb[:, 0:F - 2]) & (pb[:, 1:F - 1] > pb[:, 2:F])
    p = 10.0 ** (pb / 10.0)
    ptm = np.full_like(pb, -np.inf)
    ptm[:, 1:F - 1] = 10.0 * np.log10(p[:, 0:F - 2] + p[:, 1:F - 1] + p[:, 2:F])
    ptm = np.where(cand, ptm, -np.inf)
    margin = np.full(T, np.inf)
    gap_q = np.where(cand, np.abs(ptm - q[None, :]), np.inf)
    margin = np.minimum(margin, gap_q.min(axis=1))
    rem = cand & ~(ptm < q[None, :])
    tm = np.where(rem, ptm, -np.inf)
    surv = rem.copy()
    for k in range(1, F - 1):
        rows = rem[:, k]
        if not rows.any():
            continue
        w = tm[:, lo[k]:hi[k] + 1]
        j = np.arange(lo[k], hi[k] + 1)
        mine = tm[:, k:k + 1]
        beat = (w > mine) | ((w == mine) & (j[None, :] < k))
        surv[:, k] &= ~beat.any(axis=1)
        # the decision's own gap: a survivor is as safe as its closest rival, a suppressed candidate as its loudest one
        other = rem[:, lo[k]:hi[k] + 1] & (j[None, :] != k)
        with np.errstate(invalid="ignore"):
            d = np.where(other, w - mine, np.nan)
        has = other.any(axis=1) & rows
        if has.any():
            with np.errstate(invalid="ignore"):
                gap = np.where(surv[:, k], -np.nanmax(d, axis=1, initial=-np.inf), np.nanmax(d, axis=1, initial=-np.inf))
            margin = np.where(has, np.minimum(margin, np.abs(gap)), margin)
    theta = np.empty_like(pb)
    athl = np.where(np.arange(F) >= kA, 10.0 ** (np.nan_to_num(ath) / 10.0), 0.0)
    for t in range(T):
        js = np.nonzero(surv[t])[0]
        s = athl.copy()
        if js.size:
            dz = z[None, :] - z[js, None]
            up = -27.0 + 0.37 * np.maximum(ptm[t, js] - 40.0, 0.0)
            sf = np.where(dz <= 0, 27.0 * dz, up[:, None] * dz)
            Tj = ptm[t, js, None] - 6.025 - 0.275 * z[js, None] + sf
            s = s + (10.0 ** (Tj / 10.0)).sum(axis=0)
        with np.errstate(divide="ignore"):
            theta[t] = 10.0 * np.log10(s)
    return theta, margin, surv.sum(axis=1), surv


def threshold(x, sr=16000):
    """Clean clip (L,) -> (pbar, theta, pmax) from its own float64 STFT."""
    P, pmax = levels(x)
    pbar = P - pmax + 96.0
    theta = threshold_from_pbar(pbar, sr)[0]
    return pbar, theta, pmax


def bound(theta, pmax, margin_db=0.0):
    """A = 10^((theta + m - 96 + Pmax) / 20); 0 where theta = -inf."""
    with np.errstate(over="ignore"):
        return 10.0 ** ((np.asarray(theta, dtype=np.float64) + margin_db - 96.0 + pmax) / 20.0)


def project(delta, A, L=None):
    """delta (L,), A (T, F) -> iSTFT(S min(1, A / |S|)) aligned to L (samples from hop (T - 1) on are zero)."""
    delta = np.asarray(delta, dtype=np.float64)
    L = delta.shape[-1] if L is None else L
    S = stft_tf(delta)
    mag = np.abs(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(mag > 0, np.minimum(1.0, A / mag), 1.0)
    y = OP.compute_istft(torch.from_numpy((S * sc).T[None].astype(np.complex64)), _args())
    return OP.align_to(L, y)[0].numpy().astype(np.float64)


def _args():
    return OP.default_args(n_fft=N_FFT, hop_length=HOP, win_length=N_FFT)
