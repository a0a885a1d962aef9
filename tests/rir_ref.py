"""Reference statements of the room-response layer (include/paa_hip.h) in numpy float64: the causal FIR
``apply``, its adjoint, the magnitude sums of the error bound and the draw of the room index.  Test infrastructure only."""
import numpy as np

import place_ref as PR


def rooms(index, N):
    """Indices outside [0, N) are reduced modulo N, as the device does."""
    return np.mod(np.asarray(index, dtype=np.int64), int(N))


def apply64(bank, index, x):
    """out[b][i] = sum_{k <= min(K-1, i)} h_c[k] x[b][i-k], c = index[b] mod N; float64 (B, L)."""
    bank, x = np.asarray(bank, dtype=np.float64), np.asarray(x, dtype=np.float64)
    L = x.shape[1]
    return np.stack([np.convolve(x[b], bank[c])[:L] for b, c in enumerate(rooms(index, bank.shape[0]))])


def adjoint64(bank, index, g):
    """out[b][j] = sum_{k <= min(K-1, L-1-j)} h_c[k] g[b][j+k]; float64 (B, L)."""
    bank, g = np.asarray(bank, dtype=np.float64), np.asarray(g, dtype=np.float64)
    L = g.shape[1]
    return np.stack([np.convolve(g[b][::-1], bank[c])[:L][::-1] for b, c in enumerate(rooms(index, bank.shape[0]))])


def bound(bank, index, x, adjoint=False):
    """Per output: (K + 64) 2^-24 sum_k |h_k x| + 2^-149, the fmaf-chain bound for the padded chain length."""
    K = np.asarray(bank).shape[1]
    mag = (adjoint64 if adjoint else apply64)(np.abs(np.asarray(bank, dtype=np.float64)), index, np.abs(np.asarray(x, dtype=np.float64)))
    return (K + 64) * 2.0 ** -24 * mag + 2.0 ** -149


def draw_room(seed, step, clip_id, stream, N):
    """(r0 * N) >> 32 of Philox counter (step, clip, stream, 1): word 3 = 1 keeps it apart from placement's draws (word 3 = 0)."""
    r0 = PR.philox4x32_10((step, clip_id, stream, 1), (seed & PR.MASK, (seed >> 32) & PR.MASK))[0]
    return (r0 * int(N)) >> 32


def draw(seed, step, clip_base, B, stream, N):
    return np.array([draw_room(seed, step, clip_base + b, stream, N) for b in range(B)], dtype=np.int64)
