"""numpy statement of paa_clip_search (include/paa_hip.h): per clip, decide success from the step's word-error
counters with exact integer compares, keep the row and its scale, shrink the scale in float32."""
import numpy as np


def success(counts, targeted: bool, wer_milli: int) -> np.ndarray:
    """(B,) bool from counts (B, 3) int (errors, reference words, hypothesis words)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    e, w = c[:, 0], c[:, 1]
    if targeted:
        return (e == 0) & (w > 0)
    return (w > 0) & (e * 1000 >= np.int64(wer_milli) * w)


def shrink_scale(scale, shrink, floor_scale) -> np.ndarray:
    """fmaxf(s * shrink, floor) with every operand and the product rounded to float32."""
    s = np.asarray(scale, dtype=np.float32)
    return np.maximum(s * np.float32(shrink), np.float32(floor_scale)).astype(np.float32)


def clip_search(delta, counts, targeted, wer_milli, shrink, floor_scale, scale, best, best_scale, best_step, step):
    """One call on copies: returns (scale, best, best_scale, best_step, step) after it; the inputs are left alone."""
    delta = np.asarray(delta, dtype=np.float32)
    scale, best = np.array(scale, dtype=np.float32), np.array(best, dtype=np.float32)
    best_scale, best_step = np.array(best_scale, dtype=np.float32), np.array(best_step, dtype=np.int32)
    ok = success(counts, targeted, wer_milli)
    best[ok] = delta[ok]
    best_scale[ok] = scale[ok]
    best_step[ok] = np.int32(step)
    scale[ok] = shrink_scale(scale[ok], shrink, floor_scale)
    return scale, best, best_scale, best_step, int(step) + 1
