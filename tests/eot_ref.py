"""Reference statements of the two ends of the per-clip playback chain and of the vote over a clip's draws (include/paa_hip.h at
paa_eot_rows) in numpy: B clips, G draws each, R = B * G rows, r = b * G + g.  Test infrastructure only."""
import numpy as np


def rows32(clean, delta, gain, G):
    """rows[r] = a_r * (clean[b] + delta[b]) in float32: ONE f32 add, then ONE f32 multiply (numpy rounds each operation).
    ``clean`` None: no add; ``gain`` None: no multiply."""
    s = np.asarray(delta, dtype=np.float32)
    if clean is not None:
        s = (np.asarray(clean, dtype=np.float32) + s).astype(np.float32)
    rows = np.repeat(s, int(G), axis=0)
    if gain is not None:
        rows = (np.asarray(gain, dtype=np.float32).reshape(-1)[:, None] * rows).astype(np.float32)
    return rows


def clean_rows(clean, G):
    """clean_rows[r] = clean[b]."""
    return np.repeat(np.asarray(clean, dtype=np.float32), int(G), axis=0)


def reduce64(grad_rows, gain, G):
    """grad[b] = f32(sum_g (double) a_r * (double) G[r]), g ascending; every product of two floats is exact in float64 and the sum
    of G <= 64 of them is added in the device's order, so the float32 result is bit-exact.  Returns float32 (B, L)."""
    g = np.asarray(grad_rows, dtype=np.float32).astype(np.float64)
    R, L = g.shape
    G = int(G)
    a = np.ones(R) if gain is None else np.asarray(gain, dtype=np.float32).astype(np.float64).reshape(-1)
    acc = np.zeros((R // G, L))
    for k in range(G):                                  # ascending g, as the device adds them
        acc = acc + a[k::G, None] * g[k::G]
    return acc.astype(np.float32)


def vote(counts_rows, G, targeted):
    """counts_rows (R, 3) -> (B, 3): per clip the triple of the draw with the fewest errors (untargeted) or the most errors
    (targeted); ties go to the lowest g."""
    c = np.asarray(counts_rows, dtype=np.int64).reshape(-1, int(G), 3)
    out = np.empty((c.shape[0], 3), dtype=np.int64)
    for b in range(c.shape[0]):
        best = 0
        for g in range(1, int(G)):
            if (c[b, g, 0] > c[b, best, 0]) if targeted else (c[b, g, 0] < c[b, best, 0]):
                best = g
        out[b] = c[b, best]
    return out
