"""Helpers for the -m gpu tests: run a paa_gemm descriptor on device buffers, report errors, record the library calls of a step."""
import contextlib
import ctypes as C

import numpy as np
import torch

from paa_amd import _lib


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
