"""Reference for temporal masking of the masking threshold: the decrement tables and the spread along time, the
definition verbatim.  A time of P > 0 ms lets the threshold a frame sets fall linearly in dB, by 60 dB over P ms:
w[j] = j 60 hop 1000 / (P sr) dB at lag j frames, for the lags j <= J whose decrement stays under the model's 96 dB range."""
import numpy as np

DECAY_DB, RANGE_DB = 60.0, 96.0


def lags(ms, hop=256, sr=16000):
    """J: the largest j with j*60.0*hop*1000.0 < 96.0*ms*sr, the products in double in that written order; 0 for ms = 0."""
    j = 0
    while (j + 1) * 60.0 * hop * 1000.0 < 96.0 * ms * sr:
        j += 1
    return j


def table(ms, hop=256, sr=16000):
    """float32 (J,): w[1..J], computed in double and rounded once."""
    return np.array([j * 60.0 * hop * 1000.0 / (ms * sr) for j in range(1, lags(ms, hop, sr) + 1)], dtype=np.float64).astype(np.float32)


def tables(post_ms, pre_ms, hop=256, sr=16000):
    return table(post_ms, hop, sr), table(pre_ms, hop, sr)


def _spread(theta, post_db, pre_db, dtype):
    th = np.asarray(theta, dtype=dtype)
    T = th.shape[-2]
    out = th.copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, len(post_db) + 1):          # theta(t - j) - w_post[j] for t - j >= 0
            if j < T:
                out[..., j:, :] = np.maximum(out[..., j:, :], th[..., :T - j, :] - dtype(post_db[j - 1]))
        for j in range(1, len(pre_db) + 1):           # theta(t + j) - w_pre[j] for t + j < T
            if j < T:
                out[..., :T - j, :] = np.maximum(out[..., :T - j, :], th[..., j:, :] - dtype(pre_db[j - 1]))
    return out


def spread32(theta, post_db, pre_db):
    """theta (..., T, F) float32 (-inf allowed) -> theta' float32: every term one float32 subtraction, the maximum exact."""
    return _spread(theta, np.asarray(post_db, np.float32), np.asarray(pre_db, np.float32), np.float32)


def spread64(theta, post_db, pre_db):
    """The same in float64 (the tables as given, widened)."""
    return _spread(theta, np.asarray(post_db, np.float64), np.asarray(pre_db, np.float64), np.float64)


def burst_clip():
    """A 0.3-amplitude 1 kHz burst on samples 4096..8191 of an otherwise silent 1 s clip (float64, 16000 samples)."""
    x = np.zeros(16000)
    n = np.arange(4096, 8192)
    x[4096:8192] = 0.3 * np.sin(2 * np.pi * 1000.0 * n / 16000.0)
    return x
