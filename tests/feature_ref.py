"""float64 statement of the feature-distance loss (include/paa_hip.h paa_feature_cos) in numpy: the yardstick of
tests/test_feature_ref_host.py and tests/test_gpu_feature.py.  Test infrastructure only.

    d[b][t]  = 1 - <h, r> / (|h| |r|)                          loss_b = sum_{t < T_b} d[b][t]
    dh[b][t] = -grad_scale (r / |r| - cos h / |h|) / |h|       zero rows for t >= T_b and for the pad rows

A row with |h| <= EPS or |r| <= EPS has d = 1 and a zero cotangent row: that is the definition.  ``feature_cos`` returns everything in
float64; ``rounded`` applies the entry's two roundings (d to float32 once, loss_b = the float64 sum of those float32 values)."""
import numpy as np

EPS = 1e-8


def feature_cos(h, ref, frames=None, grad_scale=1.0, T=None):
    """h (B, Ph, H), ref (B, Pr, H) with Ph, Pr >= T (default T = min(Ph, Pr)); frames (B) per-clip frame counts (clamped to [1, T])
    or None.  Returns dict(dist (B, T) float64 with zeros for t >= T_b, loss (B,) float64, dh (B, Ph, H) float64, frames (B,))."""
    h = np.asarray(h, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    B, Ph, H = h.shape
    T = min(Ph, r.shape[1]) if T is None else int(T)
    fr = np.full(B, T) if frames is None else np.clip(np.asarray(frames, dtype=np.int64), 1, T)
    dist = np.zeros((B, T))
    dh = np.zeros((B, Ph, H))
    for b in range(B):
        for t in range(int(fr[b])):
            x, y = h[b, t], r[b, t]
            nx, ny = np.sqrt(np.dot(x, x)), np.sqrt(np.dot(y, y))
            if nx <= EPS or ny <= EPS:
                dist[b, t] = 1.0
                continue
            c = np.dot(x, y) / (nx * ny)
            dist[b, t] = 1.0 - c
            dh[b, t] = -float(grad_scale) * (y / ny - c * x / nx) / nx
    return dict(dist=dist, loss=dist.sum(axis=1), dh=dh, frames=fr)


def rounded(out):
    """(dist float32, loss float32) as the entry rounds them: d once, loss_b from the float64 sum of the rounded d."""
    d32 = out["dist"].astype(np.float32)
    return d32, d32.astype(np.float64).sum(axis=1).astype(np.float32)
