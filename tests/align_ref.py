"""float64 statement of the alignment-margin loss (include/paa_hip.h paa_align_margin) in numpy: the forced
(Viterbi) alignment of a label row to the frames on RAW logits, the per-frame hinge on that alignment and its cotangent.  The
yardstick of tests/test_align_ref_host.py, tests/test_gpu_align.py and tests/test_gpu_margin_step.py.  Test infrastructure only."""
import numpy as np

NEG = -1.0e30          # the sentinel of unreachable states (CTC_NEG of csrc/model_kernels.hip)


def extended(label_row, blank):
    """blank, l_1, blank, ..., l_S, blank for the non-negative entries l_1..l_S of the row, in order."""
    ext = [int(blank)]
    for v in np.asarray(label_row).reshape(-1):
        if v >= 0:
            ext += [int(v), int(blank)]
    return np.asarray(ext, dtype=np.int64)


def forced_alignment(z, label_row, blank, with_value=False):
    """z (T, V) float32 logits of the clip's own T frames -> pi (T,) int16, or None when no path of T frames spells the row.
    v_t(s) = z[t][e_s] + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)) in float64, one add per frame in frame order; among equal
    maxima the predecessor with the largest state index wins, at the end state 2S wins over 2S-1."""
    z = np.asarray(z, dtype=np.float32)
    T = z.shape[0]
    ext = extended(label_row, blank)
    SP = len(ext)
    skip = np.zeros(SP, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    v = np.full(SP, NEG, dtype=np.float64)
    v[0] = np.float64(z[0, ext[0]])
    if SP > 1:
        v[1] = np.float64(z[0, ext[1]])
    bp = np.zeros((T, SP), dtype=np.int8)
    for t in range(1, T):
        x1 = np.concatenate(([NEG], v[:-1]))
        x2 = np.where(skip, np.concatenate(([NEG, NEG], v[:-2]))[:SP], NEG)
        bp[t] = np.where((v >= x1) & (v >= x2), 0, np.where(x1 >= x2, 1, 2))
        v = z[t, ext].astype(np.float64) + np.maximum(v, np.maximum(x1, x2))
    s = SP - 1
    if SP >= 2 and not v[SP - 1] >= v[SP - 2]:
        s = SP - 2
    best = v[s]
    if not best > -1e29:
        return (None, best) if with_value else None
    pi = np.empty(T, dtype=np.int16)
    for t in range(T - 1, 0, -1):
        pi[t] = ext[s]
        s -= int(bp[t, s])
    pi[0] = ext[s]
    return (pi, best) if with_value else pi


def hinge(z, pi, kappa):
    """z (T, V) float32, pi (T,) -> (m (T,) float64, cstar (T,) int): m_t = (double)kappa + z[t][c*_t] - z[t][pi_t], c*_t the
    first maximum of z[t] over c != pi_t."""
    z = np.asarray(z, dtype=np.float32)
    T = z.shape[0]
    rows = np.arange(T)
    pi = np.asarray(pi, dtype=np.int64)
    masked = z.astype(np.float64)
    masked[rows, pi] = -np.inf
    cstar = np.argmax(masked, axis=1)                 # first maximum = lowest index
    m = (np.float64(np.float32(kappa)) + z[rows, cstar].astype(np.float64)) - z[rows, pi].astype(np.float64)
    return m, cstar


def align_margin(logits, labels, blank, kappa, grad_scale=1.0, frames=None, T=None):
    """logits (B, Tpad, V) float32 (rows >= T are never read), labels (B, S_max) int -> dict(loss (B,) float64, align (B, T) int16,
    dlogits (B, Tpad, V) float32, margins: per clip m over its own frames, or None).  An infeasible row: loss +inf, NaN in the
    clip's dlogits rows t < T_b, the all-blank alignment."""
    logits = np.asarray(logits, dtype=np.float32)
    B, Tpad, V = logits.shape
    T = Tpad if T is None else int(T)
    loss = np.zeros(B, dtype=np.float64)
    align = np.full((B, T), blank, dtype=np.int16)
    dl = np.zeros((B, Tpad, V), dtype=np.float32)
    margins = []
    g = np.float32(grad_scale)
    for b in range(B):
        Tb = T if frames is None else int(min(max(int(frames[b]), 1), T))
        z = logits[b, :Tb]
        pi = forced_alignment(z, labels[b], blank)
        if pi is None:
            loss[b] = np.inf
            dl[b, :Tb] = np.nan
            margins.append(None)
            continue
        m, cstar = hinge(z, pi, kappa)
        act = m > 0
        loss[b] = np.sum(np.where(act, m, 0.0))
        align[b, :Tb] = pi
        rows = np.arange(Tb)[act]
        dl[b, rows, cstar[act]] = g
        dl[b, rows, pi[act].astype(np.int64)] = -g
        margins.append(m)
    return dict(loss=loss, align=align, dlogits=dl, margins=margins)


def bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
