"""Host references for conv layer 0 (C_in = 1, k = 10, stride 5) on signals that are not white noise: a deterministic filter
bank whose rows cancel on smooth input, named test clips in closed form, and float64 / plain-float32 evaluations of the
GroupNorm statistics, the normalised activations and the per-frame LayerNorm variant.  numpy only (scipy's erf through
gemm_ref); every random number comes from paa_amd.synth's counter-based generator."""
from __future__ import annotations

import numpy as np

from gemm_ref import gelu, gelu_grad
from paa_amd import synth

K, STRIDE, SR = 10, 5, 16000
C0_GCH = 2048                                   # frames per workgroup of k_conv0_gram (csrc/model_kernels.hip)
SECOND_DIFF = slice(16, 24)                     # rows of filter_bank
TONAL = ("tone120", "tone_dc", "dc_only", "clipped")


def filter_bank(C: int = 32) -> np.ndarray:
    """[C][10] float32: 8 random rows at rule_weights' scale, the same 8 with their mean removed (zero-sum), 8 second
    differences [1, -2, 1] * g at tap offsets 0..7, 4 first differences [1, -1] * g, 4 moving averages g / 10."""
    if C != 32:
        raise ValueError("the bank has 32 rows")
    W = np.zeros((32, K), dtype=np.float32)
    rnd = synth.tensor_normal("conv0_ref.filter_bank", (8, K), std=float(np.sqrt(2.0 / K)))
    W[0:8] = rnd
    W[8:16] = rnd - rnd.mean(axis=1, keepdims=True, dtype=np.float32)
    for i in range(8):
        g = np.float32(0.5 + i / 7.0)
        W[16 + i, i:i + 3] = np.array([1.0, -2.0, 1.0], dtype=np.float32) * g
    for i, off in enumerate((0, 3, 6, 8)):
        g = np.float32(0.5 + i / 3.0)
        W[24 + i, off:off + 2] = np.array([1.0, -1.0], dtype=np.float32) * g
    for i in range(4):
        W[28 + i, :] = np.float32(0.5 + i / 3.0) / np.float32(K)
    return W


def signals(L: int) -> dict:
    """name -> float32 clip of L samples within [-1, 1] (closed forms and synth.normal only)."""
    n = np.arange(L, dtype=np.float64)
    t = n / SR
    tone = 0.5 * np.sin(2.0 * np.pi * 120.0 * t)
    dur = L / SR
    chirp = np.sin(2.0 * np.pi * (100.0 * t + (400.0 - 100.0) * t * t / (2.0 * dur)))
    gate = ((np.arange(L) // 1000) % 2 == 0).astype(np.float64)          # on / off every 1000 samples
    noise = synth.normal(synth.key_of("conv0_ref.chirp_noise"), L)
    e = synth.normal(synth.key_of("conv0_ref.lowpass"), L)
    ar = np.empty(L)
    acc = 0.0
    for i in range(L):                                                   # AR(1), a = 0.995
        acc = 0.995 * acc + e[i]
        ar[i] = acc
    out = {
        "white": synth.clean_audio(1, L)[0],
        "tone120": tone,
        "tone_dc": 0.3 * tone + 0.3,
        "chirp_gated": gate * (0.5 * chirp + 0.002 * noise),
        "lowpass": ar * (0.5 / np.abs(ar).max()),
        "dc_only": np.full(L, 0.3),
        "zeros": np.zeros(L),
        "clipped": np.clip(3.0 * tone, -1.0, 1.0),
    }
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}
    assert all(np.abs(v).max() <= 1.0 for v in out.values())
    return out


def n_frames(L: int) -> int:
    return (L - K) // STRIDE + 1


def windows(x: np.ndarray) -> np.ndarray:
    """(T0, 10) view-like copy of the frames of one clip, in the clip's dtype."""
    T0 = n_frames(x.shape[0])
    return x[np.arange(T0)[:, None] * STRIDE + np.arange(K)[None, :]]


def stats64(x, W, eps=1e-5):
    """float64 (mean, rstd) per channel over time (biased variance) of the conv of the f32 clip with the f32 weights."""
    v = np.asarray(W, dtype=np.float64) @ windows(np.asarray(x, dtype=np.float64)).T          # (C, T0)
    mean = v.mean(axis=1)
    var = ((v - mean[:, None]) ** 2).mean(axis=1)
    return mean, 1.0 / np.sqrt(var + eps)


def stats32(x, W, eps=1e-5):
    """The same evaluation entirely in float32 (f32 matmul, f32 mean and variance): the plain-f32 yardstick."""
    v = np.asarray(W, dtype=np.float32) @ np.ascontiguousarray(windows(np.asarray(x, dtype=np.float32)).T)
    assert v.dtype == np.float32
    mean = v.mean(axis=1, dtype=np.float32)
    var = ((v - mean[:, None]) ** 2).mean(axis=1, dtype=np.float32)
    return mean, np.float32(1.0) / np.sqrt(var + np.float32(eps))


def stats_err(got, ref64, eps=1e-5):
    """(e_mean, e_rstd) per channel of a (mean, rstd) pair against stats64's: |mean - mean64| / sqrt(var64 + eps) (the error as
    it lands on the normalised output) and the relative error of rstd."""
    m, r = (np.asarray(a, dtype=np.float64) for a in got)
    m64, r64 = ref64
    return np.abs(m - m64) * r64, np.abs(r - r64) / r64


def cancellation(x, W):
    """Per channel: sum_t (|w| . |x_t|)^2 / sum_t v_t^2 — how much smaller the conv output is than the terms it is summed from
    (inf where the output is exactly zero and the terms are not, 1 where both vanish)."""
    X = windows(np.asarray(x, dtype=np.float64))
    W = np.asarray(W, dtype=np.float64)
    num = ((np.abs(W) @ np.abs(X).T) ** 2).sum(axis=1)
    den = ((W @ X.T) ** 2).sum(axis=1)
    out = np.ones_like(num)
    np.divide(num, den, out=out, where=den > 0)
    out[(den == 0) & (num > 0)] = np.inf
    return out


def conv0_64(x, W, gamma, beta, eps=1e-5):
    """float64 GroupNorm (one group per channel) pre-activation y (T0, C), gelu(y), gelu'(y)."""
    v = windows(np.asarray(x, dtype=np.float64)) @ np.asarray(W, dtype=np.float64).T            # (T0, C)
    mean, rstd = stats64(x, W, eps)
    y = (v - mean) * rstd * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
    return y, gelu(y), gelu_grad(y)


def conv0_ln64(x, W, bias, gamma, beta, eps=1e-5):
    """float64 per-frame LayerNorm over the channels (the "layer" extractor): pre-activation y (T0, C) and gelu(y)."""
    v = windows(np.asarray(x, dtype=np.float64)) @ np.asarray(W, dtype=np.float64).T + np.asarray(bias, dtype=np.float64)
    mean = v.mean(axis=1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=1, keepdims=True)
    y = (v - mean) / np.sqrt(var + eps) * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
    return y, gelu(y)


def gram_stats_f32_products(x, W, eps=1e-5):
    """(mean, rstd) in the arithmetic k_conv0_gram had before its products were formed in double: chunks of 2048 frames, frame t
    of a chunk owned by thread t mod 256, every product x_j * x_q rounded to f32 and a thread's <= 8 frames summed in f32, the
    rest (threads, chunks, the two quadratic forms, the variance) in f64.  A statement about arithmetic, not the library."""
    X = windows(np.asarray(x, dtype=np.float32))
    T0 = X.shape[0]
    W = np.asarray(W, dtype=np.float64)
    G = np.zeros((K, K))
    S = np.zeros(K)
    for c0 in range(0, T0, C0_GCH):
        Xc = X[c0:c0 + C0_GCH]
        accG = np.zeros((256, K, K), dtype=np.float32)
        accS = np.zeros((256, K), dtype=np.float32)
        for r in range(0, Xc.shape[0], 256):                             # a thread's frames in the order it visits them
            blk = Xc[r:r + 256]
            accG[:blk.shape[0]] += blk[:, :, None] * blk[:, None, :]     # f32 product, f32 sum
            accS[:blk.shape[0]] += blk
        G += accG.astype(np.float64).sum(axis=0)
        S += accS.astype(np.float64).sum(axis=0)
    mean = (W @ S) / T0
    var = np.maximum(np.einsum("cj,jq,cq->c", W, G, W) / T0 - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)
