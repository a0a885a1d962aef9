"""-m gpu: CTC with a per-clip frame count (paa_ctc_len, csrc/model_kernels.hip).  No tolerance: clip b at
T_b frames runs the recursion paa_ctc runs for that clip alone at T = T_b (the work layout keeps the stride of the full T, the
arithmetic per state is the same), so nll and dlogits rows < T_b agree bit for bit, and rows beyond are zero."""
import numpy as np
import pytest
import torch

from paa_amd import _lib

pytestmark = pytest.mark.gpu

B, T, V, BLANK = 3, 24, 32, 0
FRAMES = [24, 9, 1]
NAN32 = 0x7FC00123


def _labels(S_max, rng, lens):
    lab = np.full((B, S_max), -1, dtype=np.int32)
    for b, n in enumerate(lens):
        lab[b, :n] = rng.integers(1, V, n)
    return lab


def _ctc(logits, labels, frames=None, T_=None):
    """paa_ctc (frames None) or paa_ctc_len on host arrays -> (nll, dlogits) host arrays; dlogits starts as a NaN sentinel."""
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    Bn, Tn = logits.shape[0], logits.shape[1] if T_ is None else T_
    S = labels.shape[1]
    lg = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels)).cuda()
    work = torch.zeros(int(L.paa_ctc_work_floats(Bn, Tn, V, S)), dtype=torch.float32, device="cuda")
    nll = torch.zeros(Bn, dtype=torch.float32, device="cuda")
    dl = torch.full((Bn, Tn, V), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)
    if frames is None:
        _lib.check(L.paa_ctc(p(lg), p(lab), Bn, Tn, V, S, BLANK, 1.0, p(nll), p(dl), p(work), st))
    else:
        fr = torch.tensor(frames, dtype=torch.int32, device="cuda")
        _lib.check(L.paa_ctc_len(p(lg), p(lab), p(fr), Bn, Tn, V, S, BLANK, 1.0, p(nll), p(dl), p(work), st))
    torch.cuda.synchronize()
    return nll.cpu().numpy(), dl.cpu().numpy()


# S_max 8: one state per lane (k_ctc_rec<1>); 40: one wave per state slot (k_ctc_rec_mw<2, 1>); 300: two slots per wave
# (k_ctc_rec_mw<16, 2>); 600: the block-level kernel.  Label lengths: feasible in 24 / 9 frames, and one label for the one-frame clip.
@pytest.mark.parametrize("S_max", [8, 40, 300, 600])
def test_ctc_len_equals_the_clip_alone(S_max):
    rng = np.random.default_rng(S_max)
    logits = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    labels = _labels(S_max, rng, [7, 4, 1])
    nll, dl = _ctc(logits, labels, FRAMES)
    assert np.isfinite(nll).all()
    for b, tb in enumerate(FRAMES):
        one_nll, one_dl = _ctc(logits[b:b + 1, :tb], labels[b:b + 1])
        assert nll[b:b + 1].view(np.uint32) == one_nll.view(np.uint32), (b, float(nll[b]), float(one_nll[0]))
        assert np.array_equal(dl[b, :tb].view(np.uint32), one_dl[0].view(np.uint32)), b
        assert (dl[b, tb:].view(np.uint32) == 0).all(), (b, "rows beyond T_b must be zero")


def test_ctc_len_null_and_full_frames_are_paa_ctc():
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    labels = _labels(8, rng, [7, 4, 1])
    ref = _ctc(logits, labels)
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    lg, lab = torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()
    work = torch.zeros(int(L.paa_ctc_work_floats(B, T, V, 8)), dtype=torch.float32, device="cuda")
    nll, dl = torch.zeros(B, device="cuda"), torch.zeros(B, T, V, device="cuda")
    _lib.check(L.paa_ctc_len(p(lg), p(lab), None, B, T, V, 8, BLANK, 1.0, p(nll), p(dl), p(work), st))
    torch.cuda.synchronize()
    assert np.array_equal(nll.cpu().numpy().view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(dl.cpu().numpy().view(np.uint32), ref[1].view(np.uint32))
    full = _ctc(logits, labels, [T] * B)
    assert np.array_equal(full[0].view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(full[1].view(np.uint32), ref[1].view(np.uint32))


def test_ctc_len_infeasible_clip_is_inf():
    """A label row longer than the clip's frame count is infeasible: +inf, as paa_ctc gives for that clip alone."""
    rng = np.random.default_rng(9)
    logits = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = _labels(8, rng, [7, 4, 3])                      # 3 labels in 1 frame
    nll, dl = _ctc(logits, labels, FRAMES)
    assert np.isfinite(nll[:2]).all() and np.isinf(nll[2]) and nll[2] > 0
    assert (dl[2, 1:].view(np.uint32) == 0).all()
