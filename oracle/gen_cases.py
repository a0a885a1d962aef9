"""ORACLE tooling — the case list shared by oracle/gen_goldens.py (which runs the reference) and
the tests (which never do)."""
from __future__ import annotations

from paa_amd import arch as A

from . import projections as OP

# (norm_type, extra CLI flags) — reference defaults plus the BASELINE.json epsilons.
NORM_CASES = [
    ("l2", []), ("linf", []), ("snr", ["--snr_db", "40"]), ("snr", []), ("tv", []),
    ("min_max_freqs", []), ("fletcher_munson", ["--fm_epsilon", "2.0"]),
    ("fletcher_munson", ["--fm_epsilon", "0.05"]), ("max_phon", []), ("max_phon", ["--max_phon_level", "25"]),
]
LENGTHS = [4096, 5000]
AMPS = [1e-4, 1e-2, 0.3]

PGD_CASES = [
    # name, arch, L, B, norm, extra flags
    ("tiny_group_snr", A.tiny("group", False), 8000, 3, "snr", ["--snr_db", "40"]),
    ("tiny_group_maxphon", A.tiny("group", False), 8000, 2, "max_phon", []),
    ("tiny_layer_stable_fm", A.tiny("layer", True), 8000, 2, "fletcher_munson", ["--fm_epsilon", "0.05"]),
    ("tiny_group_targeted_linf", A.tiny("group", False), 8000, 2, "linf",
     ["--attack_mode", "targeted", "--target", "ab", "--target_reps", "2"]),
    ("base_snr", A.BASE, 16000, 2, "snr", ["--snr_db", "40"]),
    # clip lengths off the 8000-multiple grid (ODD_LENGTHS): tail tiles / uncovered samples reach the reference goldens
    ("tiny_group_snr_10250", A.tiny("group", False), 10250, 3, "snr", ["--snr_db", "40"]),
    ("tiny_layer_stable_fm_8737", A.tiny("layer", True), 8737, 2, "fletcher_munson", ["--fm_epsilon", "0.05"]),
    ("base_snr_10563", A.BASE, 10563, 2, "snr", ["--snr_db", "40"]),
]
# the one PGD case whose golden holds stride-13 / stride-7 samples of grad, p_new and logits; every other case stores them whole
PGD_SAMPLED = {"base_snr"}

# Clip lengths the model tests run at.  The engine crops / pads every clip to a length taken from the data
# (build.percentile_length), so any L >= 400 reaches the kernels; the 8000-multiples alone all fall in one residue class
# of every tail below.  For the shared conv stack (k = 10,3,3,3,3,2,2; s = 5,2,2,2,2,2,2):
#   T0 % 32       conv0 frames in the last k_conv0_dgrad_dma tile (DG_T = 32): rows it re-reads and zeroes
#   T0 % 4        frames in the four-frame walk of k_conv0_gn's last chunk (C0_TCH = 128)
#   gram tail     frames in the last k_conv0_gram chunk (C0_GCH = 2048)
#   pad0          padded conv0 rows P0 - T0 (0: conv1's last, padded, row reads one row past the clip's block)
#   uncovered     waveform samples after the last conv0 window (their gradient is exactly 0)
#   T_e % 32      attention rows in the last 32-row block (Tp); T_e = 1 is a one-frame clip
#   L % 4         row alignment of the per-clip perturbation rows (row b starts at b * L floats)
ODD_LENGTHS = [
    # L, why
    (8000, "control: the grid the suite ran on (T0 % 32 = 31, one pad row, L % 4 = 0)"),
    (8166, "T0 % 32 = 0 with 32 padded conv0 rows; 1 uncovered sample; L % 4 = 2"),
    (8737, "T0 % 32 = 18, T0 % 4 = 2; 2 uncovered samples; L % 4 = 1"),
    (10245, "P0 == T0 (no conv0 pad row); full 2048-frame gram chunk; T0 % 32 = 0"),
    (10250, "T0 % 32 = 1: 31 zeroed dgrad rows; 1-frame gram tail; 63 padded conv0 rows"),
    (10563, "T_e % 32 = 0; 3 uncovered samples; L % 4 = 3"),
    (10885, "T_e % 32 = 1; 128-frame gram tail; P0 == T0"),
    (719, "T_e = 1; 4 uncovered samples; L % 4 = 3"),
    (400, "the shortest clip: T_e = 1, T0 = 79"),
]
PGD_TEXTS = ["ab cd", "hello", "a b c", "xyz w"]

_FLOAT = {"snr_db", "fm_epsilon", "max_phon_level", "l2_size", "linf_size", "tv_epsilon", "lr",
          "min_freq_attack", "max_freq_attack", "phon_reference_db"}
_INT = {"target_reps", "n_fft", "hop_length", "win_length", "sr"}


def case_name(norm, extra, L, B, amp):
    tag = "_".join(x.strip("-") for x in extra) or "default"
    return f"{norm}|{tag}|L{L}|B{B}|a{amp:g}"


def cli_to_args(norm, extra=()):
    """['--snr_db', '40'] -> oracle args namespace (same defaults as the reference parser)."""
    kw = {"norm_type": norm}
    it = iter(extra)
    for flag in it:
        key = flag.lstrip("-")
        val = next(it)
        kw[key] = float(val) if key in _FLOAT else int(val) if key in _INT else val
    return OP.default_args(**kw)
