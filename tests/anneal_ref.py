"""numpy statement of paa_clip_anneal (include/paa_hip.h): per clip, decide success as paa_clip_search does, keep the
row where its masking loss improves on the best so far (strict float32 compare), move alpha on the periods of n = step + 1 with
float32 products and float32 fmax / fmin."""
import numpy as np

from search_ref import success


def move_alpha(alpha, factor, alpha_min, alpha_max) -> np.ndarray:
    """fminf(fmaxf(a * factor, alpha_min), alpha_max) with every operand and the product rounded to float32."""
    a = np.asarray(alpha, dtype=np.float32)
    return np.fmin(np.fmax(a * np.float32(factor), np.float32(alpha_min)), np.float32(alpha_max)).astype(np.float32)


def clip_anneal(delta, counts, loss_rows, targeted, wer_milli, up_every, down_every, up, down, alpha_min, alpha_max, alpha, best,
                best_loss, best_alpha, best_step, step):
    """One call on copies: returns (alpha, best, best_loss, best_alpha, best_step, step) after it; the inputs are left alone."""
    delta = np.asarray(delta, dtype=np.float32)
    loss = np.asarray(loss_rows, dtype=np.float32)
    alpha, best = np.array(alpha, dtype=np.float32), np.array(best, dtype=np.float32)
    best_loss, best_alpha = np.array(best_loss, dtype=np.float32), np.array(best_alpha, dtype=np.float32)
    best_step = np.array(best_step, dtype=np.int32)
    n = int(step) + 1
    ok = success(counts, targeted, wer_milli)
    with np.errstate(invalid="ignore"):
        keep = ok & (loss < best_loss)                  # strict: NaN never keeps, an equal loss keeps the earlier delta
    best[keep] = delta[keep]
    best_loss[keep] = loss[keep]
    best_alpha[keep] = alpha[keep]                      # the alpha this delta was optimised under: before it moves
    best_step[keep] = np.int32(step)
    if n % int(up_every) == 0:
        alpha[ok] = move_alpha(alpha[ok], up, alpha_min, alpha_max)
    if n % int(down_every) == 0:
        alpha[~ok] = move_alpha(alpha[~ok], down, alpha_min, alpha_max)
    return alpha, best, best_loss, best_alpha, best_step, int(step) + 1
