"""Reference statements of the placement layer (include/paa_hip.h) in Python / numpy: Philox4x32-10, the
draw of (shift, gain) per clip, the gather ``place`` and its adjoint ``reduce``.  Test infrastructure only."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
LOG2_10_OVER_20 = np.float32(0.16609640474436813)


def philox4x32_10(counter, key):
    """counter: 4 uint32, key: 2 uint32 -> 4 uint32 (Salmon et al. 2011, ten rounds)."""
    c0, c1, c2, c3 = (int(x) & MASK for x in counter)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw_raw(seed, step, clip_id, stream):
    return philox4x32_10((step, clip_id, stream, 0), (seed & MASK, (seed >> 32) & MASK))


def draw_shift(seed, step, clip_id, stream, Lp, shift_on=True):
    return (draw_raw(seed, step, clip_id, stream)[0] * int(Lp)) >> 32 if shift_on else 0


def draw_gain_db(seed, step, clip_id, stream, G):
    """The f32 gain_db = fmaf(u, 2G, -G), u = (r1 >> 8) * 2^-24 (the product and the sum are exact in f64 for G on the f32 grid up
    to 20, so one rounding to f32 is the fused result)."""
    u = float(draw_raw(seed, step, clip_id, stream)[1] >> 8) * 2.0 ** -24
    G = float(np.float32(G))
    return np.float32(u * (2.0 * G) - G)


def draw_gain64(seed, step, clip_id, stream, G):
    """10^(gain_db / 20) in float64 on the f32 gain_db."""
    return 10.0 ** (float(draw_gain_db(seed, step, clip_id, stream, G)) / 20.0)


def draw(seed, step, clip_base, B, stream, Lp, shift_on=True, G=0.0):
    """(shifts int64 (B), gains float64 (B)) of the clips clip_base .. clip_base + B - 1."""
    s = np.array([draw_shift(seed, step, clip_base + b, stream, Lp, shift_on) for b in range(B)], dtype=np.int64)
    a = np.array([draw_gain64(seed, step, clip_base + b, stream, G) for b in range(B)], dtype=np.float64)
    return s, a


def index(L, Lp, shift):
    """(B, L) source index (i + s_b) mod Lp; shifts outside [0, Lp) are reduced modulo Lp."""
    s = np.mod(np.asarray(shift, dtype=np.int64), Lp)
    return (np.arange(L, dtype=np.int64)[None, :] + s[:, None]) % Lp


def place(p, L, shift, gain=None, dtype=np.float32):
    """rows[b][i] = a_b * p[(i + s_b) mod Lp] in ``dtype`` (float32: one f32 multiply, the device's arithmetic)."""
    p = np.asarray(p, dtype=dtype).reshape(-1)
    rows = p[index(L, p.shape[0], shift)]
    if gain is not None:
        rows = rows * np.asarray(gain, dtype=dtype)[:, None]
    return rows.astype(dtype)


def reduce64(G, shift, gain, Lp):
    """The adjoint of ``place`` in float64: (grad (Lp), sum of |terms| (Lp), term count (Lp))."""
    G = np.asarray(G, dtype=np.float64)
    B, L = G.shape
    a = np.ones(B) if gain is None else np.asarray(gain, dtype=np.float64)
    idx = index(L, Lp, shift)
    terms = G * a[:, None]
    grad = np.zeros(Lp)
    mag = np.zeros(Lp)
    cnt = np.zeros(Lp, dtype=np.int64)
    for b in range(B):
        np.add.at(grad, idx[b], terms[b])
        np.add.at(mag, idx[b], np.abs(terms[b]))
        np.add.at(cnt, idx[b], 1)
    return grad, mag, cnt
