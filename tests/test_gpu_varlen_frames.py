"""-m gpu: the small kernels of the length mode (csrc/model.hip), bit for bit: paa_zero_frames on an f32
buffer and on planar and interleaved bf16 planes, paa_mask_tail_rows, paa_argmax_ids_len.  Every buffer starts as a sentinel:
what must be zeroed is zero bits, what must not be touched keeps the sentinel; out-of-range counts are clamped on the device."""
import numpy as np
import pytest
import torch

from paa_amd import _lib

pytestmark = pytest.mark.gpu

B, T, P, COLS = 3, 11, 13, 64
FRAMES = [11, 4, 0]                       # 0 is clamped to 1
EFF = [11, 4, 1]
S32, S16 = 0x7FC00123, 0x7FC5


def _zero(x, hi, lo, il, frames):
    fr = torch.tensor(frames, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().paa_zero_frames(_lib.ptr(x), _lib.ptr(hi), _lib.ptr(lo), il, _lib.ptr(fr), B, T, P, COLS,
                                          _lib.stream_ptr()))
    torch.cuda.synchronize()


def _expected_zero():
    z = np.zeros((B, P), dtype=bool)
    for b, t in enumerate(EFF):
        z[b, t:T] = True
    return z


def test_zero_frames_f32_and_planar_planes():
    x = torch.full((B, P, COLS), S32, dtype=torch.int32, device="cuda")
    hi = torch.full((B, P, COLS), S16, dtype=torch.int16, device="cuda")
    lo = torch.full((B, P, COLS), S16, dtype=torch.int16, device="cuda")
    _zero(x.view(torch.float32), hi, lo, 0, FRAMES)
    z = _expected_zero()
    for name, t, s in (("f32", x, S32), ("hi", hi, S16), ("lo", lo, S16)):
        a = t.cpu().numpy()
        assert (a[z] == 0).all(), name
        assert (a[~z] == s).all(), name
    # planes alone (no f32 buffer), hi plane only
    hi2 = torch.full((B, P, COLS), S16, dtype=torch.int16, device="cuda")
    _zero(None, hi2, None, 0, FRAMES)
    assert torch.equal(hi2, hi)


def test_zero_frames_interleaved_planes():
    """il = 1: ONE array of twice the elements, [32 hi | 32 lo | 32 hi | ...] per 32-element group."""
    il = torch.full((B * P * COLS * 2,), S16, dtype=torch.int16, device="cuda")
    _zero(None, il, None, 1, FRAMES)
    a = il.cpu().numpy().reshape(B, P, COLS // 32, 2, 32)          # (clip, row, group, hi / lo, element)
    z = _expected_zero()
    assert (a[z] == 0).all() and (a[~z] == S16).all()


def test_zero_frames_refuses_bad_shapes():
    fr = torch.ones(B, dtype=torch.int32, device="cuda")
    x = torch.zeros(B, P, COLS, device="cuda")
    L = _lib.lib()
    for args in ((B, T, T - 1, COLS, 0), (B, T, P, 6, 0), (B, T, P, 48, 1), (0, T, P, COLS, 0)):
        b, t, p, c, il = args
        assert L.paa_zero_frames(_lib.ptr(x), _lib.ptr(x), None, il, _lib.ptr(fr), b, t, p, c, _lib.stream_ptr()) == _lib.PAA_ERR_ARG
    assert L.paa_zero_frames(None, None, None, 0, _lib.ptr(fr), B, T, P, COLS, _lib.stream_ptr()) == _lib.PAA_ERR_ARG


def test_mask_tail_rows():
    rows, L = 4, 1001
    lens = [1001, 400, 0, 5000]              # 5000 is clamped to L, 0 empties the row
    p = torch.full((rows, L), S32, dtype=torch.int32, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().paa_mask_tail_rows(_lib.ptr(p.view(torch.float32)), rows, L, _lib.ptr(ln), _lib.stream_ptr()))
    torch.cuda.synchronize()
    a = p.cpu().numpy()
    for r, n in enumerate([1001, 400, 0, 1001]):
        assert (a[r, :n] == S32).all() and (a[r, n:] == 0).all(), r


def test_argmax_ids_len():
    Bn, Tn, V, blank = 3, 9, 32, 7
    rng = np.random.default_rng(3)
    x = rng.standard_normal((Bn, Tn, V)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    fr = torch.tensor([9, 4, -2], dtype=torch.int32, device="cuda")          # -2 is clamped to 1
    ids = torch.full((Bn, Tn), -1, dtype=torch.int16, device="cuda")
    _lib.check(_lib.lib().paa_argmax_ids_len(_lib.ptr(xd), Bn, Tn, V, _lib.ptr(fr), blank, _lib.ptr(ids), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = ids.cpu().numpy()
    for b, t in enumerate([9, 4, 1]):
        assert np.array_equal(got[b, :t], x[b, :t].argmax(-1)) and (got[b, t:] == blank).all(), b
