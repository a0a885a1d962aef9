"""Float64 numpy restatement of the STFT, the iSTFT and the three spectral projections at ANY frame geometry (n_fft, hop),
win_length = n_fft: the target of the generic frame kernels (proj_kernels.hip: fft_lds, k_frame, k_ola), which every geometry
other than 1024 / 256 runs.  test_stft_ref_host.py ties it to torch.stft / torch.istft in float64 and to the float32 oracle.

Spectra are frame-major (B, T, F), as paa_stft writes them; the (B, F, T) tensor of the reference is the transposed view."""
import numpy as np

from oracle import iso226

SPECTRAL_NORMS = ("min_max_freqs", "max_phon", "fletcher_munson")

# (n_fft, hop), win_length = n_fft: both parities of log2(n_fft) (odd ones take the radix-2 pass of the LDS FFT), the ends of
# the accepted range, hops that do not divide n_fft, a hop above n_fft/2, and 1024 off the fused kernels' hop of 256
GEOMETRIES = [(64, 16), (128, 32), (256, 64), (512, 128), (512, 100), (512, 256), (512, 384), (1024, 200), (2048, 512),
              (2048, 300), (4096, 1024)]
ROWS = (1, 3, 33)
LOUD_ROW, LOUD_AMP, AMP = 1, 0.5, 0.05


def lengths(n_fft, hop):
    """The shortest accepted clip, two lengths off every grid, an exact multiple of the hop, and a 1 s clip plus one sample.
    A clip shorter than the hop has ONE frame and an empty iSTFT (of these only 257 at (512, 384)): it is not part of the sweep."""
    out = [n_fft // 2 + 1, n_fft + 37, 5 * n_fft + 3, hop * (2 * (n_fft // hop) + 3), 16001]
    return [L for L in out if L >= hop]


def signal(n_fft, hop, L, rows=max(ROWS)):
    """Seeded randn * 0.05; row LOUD_ROW at amplitude 0.5 (max_phon clips most of its bins)."""
    rng = np.random.default_rng([n_fft, hop, L])
    x = rng.standard_normal((rows, L)) * AMP
    if rows > LOUD_ROW:
        x[LOUD_ROW] *= LOUD_AMP / AMP
    return x.astype(np.float32)


def random_spectrum(n_fft, hop, L, rows=max(ROWS)):
    """(rows, T, F) complex64 that is NOT the STFT of a signal: independent frames, Im(DC) and Im(Nyquist) non-zero."""
    rng = np.random.default_rng([n_fft, hop, L, 1])
    shape = (rows, n_frames(L, hop), n_fft // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def geometry_args(norm, n_fft, hop, **kw):
    """The oracle's argument namespace at a frame geometry; min_max_freqs at n_fft = 512 puts both ends exactly on a bin."""
    from oracle import projections as OP
    if norm == "min_max_freqs" and n_fft == 512:
        kw = dict(min_freq_attack=500.0, max_freq_attack=3000.0, **kw)
    return OP.default_args(norm_type=norm, n_fft=n_fft, hop_length=hop, win_length=n_fft, **kw)


def hann(n_fft):
    """Periodic Hann evaluated in float64, ROUNDED TO FLOAT32 and widened again: the kernels read the window from a float32
    table (paa_proj_create), so the rounded samples are the operation's definition, not part of its error."""
    k = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / n_fft)).astype(np.float32).astype(np.float64)


def n_frames(L, hop):
    return 1 + L // hop


def stft(x, n_fft, hop, window=None):
    """(B, L) -> (B, T, F) complex128: reflect pad n_fft/2 (center=True), frame t starts at t * hop, T = 1 + L // hop."""
    x = np.asarray(x, dtype=np.float64)
    B, L = x.shape
    if L <= n_fft // 2:
        raise ValueError(f"L={L} must exceed n_fft/2={n_fft // 2} (reflect padding)")
    w = hann(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    T = n_frames(L, hop)
    idx = (np.arange(T) * hop)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(xp[:, idx] * w, axis=-1)


def envelope(T, n_fft, hop, window=None):
    """Overlap-added squared window over the n_fft + hop * (T - 1) padded samples."""
    w = hann(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    env = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        env[t * hop:t * hop + n_fft] += w * w
    return env


def istft(S, n_fft, hop, window=None):
    """(B, T, F) -> (B, hop * (T - 1)): Im(DC) and Im(Nyquist) dropped (a real inverse transform cannot see them), irfft,
    window, overlap-add, division by the summed squared window, n_fft/2 trimmed from both ends."""
    S = np.array(S, dtype=np.complex128)
    B, T, F = S.shape
    if F != n_fft // 2 + 1:
        raise ValueError(f"{F} bins, expected {n_fft // 2 + 1}")
    if T < 2:
        raise ValueError("one frame: hop * (T - 1) = 0 samples")
    w = hann(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    S[..., 0] = S[..., 0].real
    S[..., -1] = S[..., -1].real
    y = np.fft.irfft(S, n=n_fft, axis=-1) * w
    total = n_fft + hop * (T - 1)
    out = np.zeros((B, total))
    for t in range(T):
        out[:, t * hop:t * hop + n_fft] += y[:, t]
    half = n_fft // 2
    return out[:, half:total - half] / envelope(T, n_fft, hop, w)[half:total - half]


def align_to(length, y):
    """_align_to: right zero-pad or crop the last axis to ``length``."""
    if y.shape[-1] >= length:
        return y[..., :length]
    return np.pad(y, ((0, 0), (0, length - y.shape[-1])))


def bin_freqs(n_fft, sr):
    return np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)


def min_max_freqs(S, n_fft, sr, min_freq, max_freq):
    """Keeps only the bins OUTSIDE [min, max]; a bin exactly on either end is inside, so it is zeroed."""
    f = bin_freqs(n_fft, sr)
    return S * ((f < min_freq) | (f > max_freq))


def max_phon(S, spl_thresh, phon_reference_db):
    """Every bin rebuilt from (clipped dB magnitude, phase)."""
    spl = np.asarray(spl_thresh, dtype=np.float64).reshape(-1)
    mag_db = 20.0 * np.log10(np.abs(S) + 1e-8)
    thr = spl - spl.max() + float(phon_reference_db)
    mag = 10.0 ** (np.minimum(mag_db, thr) / 20.0)
    return mag * np.exp(1j * np.angle(S))


def fm_row_power(S, n_fft, sr):
    """(B,): sum over a row's bins of |S|^2 w(10 log10(|S|^2 + 1e-10), f_bin), w the bilinear ISO-226 weight (1 outside the
    grid)."""
    power = np.abs(S) ** 2
    spl = 10.0 * np.log10(power + 1e-10)
    f = np.broadcast_to(bin_freqs(n_fft, sr), S.shape)
    w = iso226.interp_weights(np.stack([spl.reshape(-1), f.reshape(-1)], axis=-1)).reshape(S.shape)
    return (power * w).sum(axis=(1, 2))


def fm_norm(S, n_fft, sr):
    """The weighted norm of the WHOLE tensor: sqrt of the summed row powers."""
    return float(np.sqrt(fm_row_power(S, n_fft, sr).sum()))


def fletcher_munson(S, n_fft, sr, fm_epsilon):
    """ONE factor for the whole tensor: eps / max(norm, 1e-8) when the weighted norm exceeds eps."""
    norm = fm_norm(S, n_fft, sr)
    if norm <= fm_epsilon:
        return S
    return S * (fm_epsilon / max(norm, 1e-8))


def spectrum_project(S, norm, args, spl_thresh=None):
    n_fft, sr = int(args.n_fft), int(args.sr)
    if norm == "min_max_freqs":
        return min_max_freqs(S, n_fft, sr, float(args.min_freq_attack), float(args.max_freq_attack))
    if norm == "max_phon":
        return max_phon(S, spl_thresh, args.phon_reference_db)
    if norm == "fletcher_munson":
        return fletcher_munson(S, n_fft, sr, float(args.fm_epsilon))
    raise ValueError(f"not a spectral norm: {norm!r}")


def project(x, norm, args, spl_thresh=None):
    """perturbation_constraint for a spectral norm on (B, L): STFT -> per-bin op -> iSTFT -> _align_to(L)."""
    n_fft, hop = int(args.n_fft), int(args.hop_length)
    x = np.asarray(x, dtype=np.float64)
    S = spectrum_project(stft(x, n_fft, hop), norm, args, spl_thresh)
    return align_to(x.shape[-1], istft(S, n_fft, hop))


def project_rows(x, norm, args, spl_thresh=None):
    """Every row on its own (paa_project_rows): differs from ``project`` for fletcher_munson only."""
    return np.concatenate([project(x[r:r + 1], norm, args, spl_thresh) for r in range(x.shape[0])], axis=0)
