"""Helpers for the -m gpu tests: run a paa_gemm descriptor on device buffers, report errors, record the library calls of a step,
the rows and sizes the row-projection tests share."""
import contextlib
import ctypes as C
import types

import numpy as np
import torch

from oracle import projections as OP
from paa_amd import _lib, synth


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_gemm(d: dict, bufs: dict, offs: dict = None):
    """d: descriptor fields (ints/floats) with operand keys A,B,C,(bias,aux,residual,C_pre) naming entries of
    ``bufs`` (torch cuda float32 tensors); offs: element offsets per operand name."""
    offs = offs or {}
    desc = _lib.PaaGemmDesc()
    desc.a_kcontig = 1
    desc.b_kcontig = 1
    desc.batch = 1
    desc.batch2 = 1
    desc.alpha = 1.0
    for k, v in d.items():
        if k in ("A", "B", "C", "bias", "aux", "residual", "C_pre", "A_lo", "B_lo", "Cb", "Cb_lo"):
            t = bufs[v]
            base = {'A_lo': 'A', 'B_lo': 'B', 'Cb': 'C', 'Cb_lo': 'C', 'C_pre': 'C'}.get(k, k)
            setattr(desc, k, t.data_ptr() + t.element_size() * offs.get(k, offs.get(base, 0)))
        else:
            setattr(desc, k, v)
    _lib.check(_lib.lib().paa_gemm(C.byref(desc), _lib.stream_ptr()))
    torch.cuda.synchronize()


def rel_err(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


class _LibProxy:
    """Forwards every attribute to the loaded library; a called ``paa_*`` entry appends its name to ``names`` first.  The
    ``paa_*_destroy`` entries are left out: finalizers call them, whenever an object of an earlier test happens to be freed."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("paa_") or name.endswith("_destroy"):
            return fn

        def call(*a):
            self._names.append(name)
            return fn(*a)
        return call


@contextlib.contextmanager
def record_launches():
    """``with record_launches() as names``: every ``paa_*`` entry called through ``paa_amd._lib.lib()`` inside the block, in call
    order.  The calls themselves go through unchanged."""
    real, names = _lib.lib, []
    proxy = _LibProxy(real(), names)
    _lib.lib = lambda: proxy
    try:
        yield names
    finally:
        _lib.lib = real


# ---- rows and sizes of the row-projection tests (test_gpu_search, the parent pin of test_gpu_projections) ------------------------
# Sizes under which, with the rows of test_project_rows_vs_oracle (amplitudes 1 / 0.1 / 0.01 / 1 / 0.1) and the scales below, the
# 0.01 row (scale 0.8^3) is left alone and the others are rescaled, every row far from its projection's branch (chosen with the
# oracle on the CPU: l2 norms 127 / 12.6 / 1.28 (L = 16000) and 155 / 15.6 / 1.56 (24001); TV(p) / TV(clean) 19.8 / 2.0 / 0.20; SNR
# -26 / -6.1 / +13.9 dB; FM norms 2702 / 327 / 35.5 and 3288 / 402 / 43.2, at n_fft 512: 1975 / 237 / 25.1; max |p| 4.5 / 0.49 /
# 0.043).  phon_reference_db 0 puts the contour where the two louder rows reach it.
PROJ_ARGS = ["--l2_size", "5", "--linf_size", "0.2", "--snr_db", "5", "--tv_epsilon", "1", "--fm_epsilon", "100",
             "--phon_reference_db", "0"]
SCALES = np.array([1.0, 0.5, 0.8 ** 3, 0.01, 1.0], dtype=np.float32)
SIZE_OF = {"l2": "l2_size", "linf": "linf_size", "tv": "tv_epsilon", "fletcher_munson": "fm_epsilon"}


def rows_input(rows, L, seed=5):
    amp = np.array([10.0 ** -(r % 3) for r in range(rows)], dtype=np.float32)[:, None]
    src = np.stack([synth.normal(synth.key_of(f"rowsrc{r}", seed), L) for r in range(rows)]).astype(np.float32) * amp
    return src, synth.clean_audio(rows, L, seed=seed)


def with_(args, **kw):
    return types.SimpleNamespace(**{**vars(args), **kw})


def scaled_args(args, n, s):
    """The oracle's args of norm ``n`` with its size tightened by s."""
    s = float(s)
    if n in SIZE_OF:
        return with_(args, norm_type=n, **{SIZE_OF[n]: float(getattr(args, SIZE_OF[n])) * s})
    if n == "snr":
        return with_(args, norm_type=n, snr_db=float(args.snr_db) - 20.0 * np.log10(s))
    if n == "max_phon":
        return with_(args, norm_type=n, phon_reference_db=float(args.phon_reference_db) + 20.0 * np.log10(s))
    return with_(args, norm_type=n)


def branch(n, p, clean, a):
    """(rescaled?, distance from the branch) of the oracle's projection of ``p`` (one row, or all the rows one statistic spans) under args ``a``: relative for l2 / tv / fm,
    in dB for snr; None for the norms without a row-level branch."""
    if n == "l2":
        v, eps = float(p.norm()), a.l2_size
    elif n == "tv":
        v = float((p[:, 1:] - p[:, :-1]).abs().sum())
        eps = a.tv_epsilon * float((clean[:, 1:] - clean[:, :-1]).abs().sum())
    elif n == "fletcher_munson":
        v, eps = float(OP.fm_weighted_norm(OP.compute_stft(p, a), a)), a.fm_epsilon
    elif n == "snr":
        cur = float(10 * torch.log10((clean ** 2).mean() / ((p ** 2).mean() + 1e-12)))
        return cur < a.snr_db, abs(cur - a.snr_db) / 0.01 * 1e-4        # 0.01 dB counts as 1e-4 relative
    elif n == "linf":
        return bool((p.abs() > a.linf_size).any()), 1.0
    else:
        return None, 1.0
    return v > eps, abs(v - eps) / eps
