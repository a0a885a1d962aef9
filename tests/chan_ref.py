"""Reference statements of the playback channel (include/paa_hip.h) in numpy float64 / Python integers:
the drift resampler ``apply64``, its transpose ``adjoint64``, the error ``bound``, the ``draw`` of (ratio, SNR) per clip, the noise
samples ``noise64`` and their scale ``sigma64``.  Test infrastructure only.

Drift.  Clip b holds an unsigned Q32 ratio rq_b (r_b = rq_b / 2^32, clamped to [2^31, 2^33]); with T = 8, for 0 <= i < L

    pos_q = i * rq_b (exact),  n = pos_q >> 32,  f = (pos_q & 0xffffffff) * 2^-32
    y[i]  = sum_{t = -T+1 .. T} w(t - f) x[n + t]             x[j] = 0 outside [0, L)
    w(u)  = sinc(u) (1 + cos(pi u / T)) / 2 for |u| < T, else 0;  sinc(0) = 1

and sin(pi (t - f)) = -(-1)^t sin(pi f), so f = 0 gives the weights {1, 0, ...} exactly.

Philox layout.  Every stream is Philox4x32-10 under the run's seed, key (k0, k1) = (seed & 0xffffffff, seed >> 32):

    stream            key                    counter (word 0, 1, 2, 3)
    placement draw    (k0, k1)               (step, clip, stream_id, 0)
    room draw         (k0, k1)               (step, clip, stream_id, 1)
    channel draw      (k0, k1)               (step, clip, stream_id, 2)
    noise samples     (k0, k1 ^ NOISE_KEY)   (step, clip, i >> 2,    stream_id)

The three draws differ in counter word 3; the noise differs from all of them in the key (NOISE_KEY != 0), so no (counter, key)
pair can coincide.  Noise sample i takes the word pair (c[2p], c[2p+1]), p = (i & 3) >> 1, of its block:

    u1 = ((c[2p] >> 8) + 1) 2^-24 in (0, 1],  u2 = (c[2p+1] >> 8) 2^-24 in [0, 1),  rad = sqrt(-2 ln u1)
    z_i = rad cos(2 pi u2) for even i, rad sin(2 pi u2) for odd i
"""
import numpy as np

import place_ref as PR

T = 8
TAPS = np.arange(-T + 1, T + 1, dtype=np.int64)
RQ_ONE, RQ_MIN, RQ_MAX = 1 << 32, 1 << 31, 1 << 33
NOISE_KEY = 0x6E6F6973
TAG_PLACE, TAG_ROOM, TAG_CHAN = 0, 1, 2


def clamp_rq(rq):
    return min(max(int(rq), RQ_MIN), RQ_MAX)


def rq_of(ratio):
    """The Q32 integer of a float ratio (how ``set_channel`` pins one)."""
    return clamp_rq(int(round(float(ratio) * 2.0 ** 32)))


def drift_q32(ppm):
    """D = round(drift_ppm * 1e-6 * 2^32), the host's half of the draw."""
    return int(round(float(ppm) * 1e-6 * 2.0 ** 32))


def positions(rq, L):
    """(n int64 (L), f float64 (L), exact) of the outputs 0 .. L-1."""
    assert int(L) * RQ_MAX < 1 << 63          # int64 holds every product
    pos = np.arange(int(L), dtype=np.int64) * np.int64(clamp_rq(rq))
    return pos >> 32, (pos & 0xFFFFFFFF).astype(np.float64) * 2.0 ** -32


def sinpi(f):
    """sin(pi f) for f in [0, 1] without the rounding of pi * f near f = 1: sin(pi f) = sin(pi (1 - f)), and 1 - f is exact there."""
    f = np.asarray(f, dtype=np.float64)
    return np.sin(np.pi * np.where(f > 0.5, 1.0 - f, f))


def w64(t, f):
    """w(t - f) in float64 by the sign identity: exactly {1, 0, ...} at f = 0."""
    t, f = np.broadcast_arrays(np.asarray(t, dtype=np.int64), np.asarray(f, dtype=np.float64))
    u = t - f
    sign = np.where(t & 1, 1.0, -1.0)
    safe = np.where(u == 0, 1.0, u)
    w = sign * sinpi(f) / (np.pi * safe) * 0.5 * (1.0 + np.cos(np.pi * u / T))
    return np.where(u == 0, 1.0, np.where(np.abs(u) < T, w, 0.0))


def w32(t, f):
    """The float32 weights of the kernels, rounding by rounding, with correctly rounded float32 sinpi / cospi:
    u = fl32(t - f);  1 at u = 0, 0 at |u| >= T;  else fl32(+-sinpi32(f) (0.5 + 0.5 cospi32(u / 8)) / (pi u)), the combination
    carried in float64 and rounded once."""
    t, f = np.broadcast_arrays(np.asarray(t, dtype=np.int64), np.asarray(f, dtype=np.float32))
    u = t.astype(np.float32) - f
    s = sinpi(f.astype(np.float64)).astype(np.float32)
    c0 = np.cos(np.pi * (u * np.float32(0.125)).astype(np.float64)).astype(np.float32)
    c = 0.5 + 0.5 * c0.astype(np.float64)
    num = np.where(t & 1, s, -s).astype(np.float64)
    safe = np.where(u == 0, np.float32(1), u).astype(np.float64)
    w = ((num * c) / (np.pi * safe)).astype(np.float32)
    return np.where(u == 0, np.float32(1), np.where(np.abs(u) < T, w, np.float32(0))).astype(np.float32)


def _clip(rq, x, wfun, adjoint):
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    n, f = positions(rq, L)
    idx = n[:, None] + TAPS[None, :]                          # (L, 16): column of the matrix row i
    ok = (idx >= 0) & (idx < L)
    W = wfun(TAPS[None, :], f[:, None]) * ok
    idc = np.clip(idx, 0, L - 1)
    if not adjoint:
        return (W * x[idc]).sum(axis=1)
    out = np.zeros(L)
    np.add.at(out, idc[ok], (W * x[:, None])[ok])
    return out


def apply64(rq, x):
    """y (B, L) float64; ``rq``: one Q32 integer per row."""
    return np.stack([_clip(r, xb, w64, False) for r, xb in zip(rq, np.asarray(x, dtype=np.float64))])


def adjoint64(rq, g):
    """gx[j] = sum_{i : n_i in [j-T, j+T-1]} w(j - n_i - f_i) g[i]: the transpose of ``apply64``."""
    return np.stack([_clip(r, gb, w64, True) for r, gb in zip(rq, np.asarray(g, dtype=np.float64))])


def bound(rq, x, adjoint=False):
    """Per output 2^-24 (16 sum |w x| + 8 sum |x|) + 2^-149, the sums over the terms of that output: the 16-term fmaf chain, and
    the rounding of the float32 weights (``w32``: at most 2.25 units with correctly rounded sinpi / cospi, 1.6 measured; the rest
    is f's own rounding to float32 and margin for the device's transcendentals)."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    one = lambda t, f: np.ones(np.broadcast(t, f).shape)
    absw = lambda t, f: np.abs(w64(t, f))
    mag_w = np.stack([_clip(r, xb, absw, adjoint) for r, xb in zip(rq, ax)])
    mag_1 = np.stack([_clip(r, xb, one, adjoint) for r, xb in zip(rq, ax)])
    return 2.0 ** -24 * (16.0 * mag_w + 8.0 * mag_1) + 2.0 ** -149


def key_of(seed, noise=False):
    k0, k1 = seed & PR.MASK, (seed >> 32) & PR.MASK
    return (k0, k1 ^ NOISE_KEY) if noise else (k0, k1)


def draw_counter(step, clip_id, stream):
    return (step & PR.MASK, clip_id & PR.MASK, stream & PR.MASK, TAG_CHAN)


def noise_counter(step, clip_id, group, stream):
    return (step & PR.MASK, clip_id & PR.MASK, group & PR.MASK, stream & PR.MASK)


def draw_one(seed, step, clip_id, stream, D, lo, hi):
    """(rq: Python int, snr_db: float32) of one clip: rq = 2^32 + ((c0 - 2^31) D >> 31) in integers (>> floors, as the device's
    arithmetic shift), snr_db = fmaf(u, hi - lo, lo) with u = (c1 >> 8) 2^-24 and hi - lo rounded to float32 first."""
    c = PR.philox4x32_10(draw_counter(step, clip_id, stream), key_of(seed))
    rq = RQ_ONE + (((c[0] - (1 << 31)) * int(D)) >> 31)
    u = float(c[1] >> 8) * 2.0 ** -24
    span = np.float32(np.float32(hi) - np.float32(lo))
    return rq, np.float32(u * float(span) + float(np.float32(lo)))


def draw(seed, step, clip_base, B, stream, D, lo=0.0, hi=0.0):
    """(rq: list of B Python ints, snr_db: float32 (B)) of the clips clip_base .. clip_base + B - 1."""
    both = [draw_one(seed, step, clip_base + b, stream, D, lo, hi) for b in range(B)]
    return [r for r, _ in both], np.array([s for _, s in both], dtype=np.float32)


def noise_uniforms(seed, step, clip_id, stream, L):
    """(u1 (L), u2 (L)) float64, exact: what Box-Muller reads for every sample."""
    u1, u2 = np.empty(L), np.empty(L)
    for g in range((L + 3) // 4):
        c = PR.philox4x32_10(noise_counter(step, clip_id, g, stream), key_of(seed, True))
        for p in range(2):
            a, b = ((c[2 * p] >> 8) + 1) * 2.0 ** -24, (c[2 * p + 1] >> 8) * 2.0 ** -24
            for i in (4 * g + 2 * p, 4 * g + 2 * p + 1):
                if i < L:
                    u1[i], u2[i] = a, b
    return u1, u2


def noise64(seed, step, clip_id, stream, L):
    """z (L) float64, standard normal by Box-Muller."""
    u1, u2 = noise_uniforms(seed, step, clip_id, stream, int(L))
    rad = np.sqrt(-2.0 * np.log(u1))
    even = (np.arange(int(L)) & 1) == 0
    return rad * np.where(even, np.cos(2.0 * np.pi * u2), np.sin(2.0 * np.pi * u2))


def sigma64(clean, snr_db):
    """sigma_b = sqrt(mean_i clean[b][i]^2) 10^(-snr_b / 20); float64 (B)."""
    clean = np.asarray(clean, dtype=np.float64)
    return np.sqrt((clean * clean).mean(axis=1)) * 10.0 ** (-np.asarray(snr_db, dtype=np.float64) / 20.0)
