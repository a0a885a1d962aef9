"""-m gpu: forced alignment and the alignment-margin loss through the C ABI (paa_align_margin, csrc/model_kernels.hip; DESIGN.md
§6l) against the float64 statement tests/align_ref.py.

Tolerances (derived, not measured):
  align, dlogits  exact.  Both sides run the same IEEE float64 adds and maxima in the same order (one add per frame on raw
                  logits, no transcendentals), so the path values are the same bits and the tie rule alone decides equal
                  maxima; the cotangent is 0 / +-g.
  loss            2^-22 relative: a float64 sum of at most 4096 non-negative terms (relative error <= 4096 * 2^-53 whatever the
                  order) rounded once to float32 (2^-24), with slack.
Every output sits between guard blocks that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_ref as AR
from paa_amd import _lib

pytestmark = pytest.mark.gpu

BLANK = 0
GUARD = 64                      # elements of guard on either side of every output
G32, G16 = 0x7FC00ABC, 0x7B7B
LOSS_RTOL = 2.0 ** -22


class _Guarded:
    """n elements of `dtype` between two guard blocks, every element (the payload too) preset to a recognisable pattern."""

    def __init__(self, n, dtype, pattern):
        self.n, self.pattern = n, pattern
        self.buf = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def read(self):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == self.pattern).all() and (h[GUARD + self.n:] == self.pattern).all(), "guard block overwritten"
        return h[GUARD:GUARD + self.n].copy()


def run(logits, labels, T=None, frames=None, kappa=1.0, g=1.0, want_dl=True, want_align=True, want_planes=True, calls=1):
    """paa_align_margin on host arrays: logits (B, Tpad, V), labels (B, S_max).  Returns dict(loss f32 (B,), align (B, T) int16 |
    None, dlogits f32 (B, Tpad, V) | None, hi / lo uint16 planes | None)."""
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    B, Tpad, V = logits.shape
    T = Tpad if T is None else T
    S = labels.shape[1]
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device="cuda")
    nw = int(L.paa_align_margin_work_floats(B, T, V, S))
    assert nw > 0
    work = _Guarded(nw, torch.int32, G32)
    loss = _Guarded(B, torch.int32, G32)
    al = _Guarded(B * T, torch.int16, G16) if want_align else None
    dl = _Guarded(B * Tpad * V, torch.int32, G32) if want_dl else None
    hi = _Guarded(B * Tpad * V, torch.int16, G16) if want_dl and want_planes else None
    lo = _Guarded(B * Tpad * V, torch.int16, G16) if want_dl and want_planes else None
    opt = lambda x: None if x is None else x.ptr()
    for _ in range(calls):
        _lib.check(L.paa_align_margin(p(lg), p(lab), p(fr), B, T, Tpad, V, S, BLANK, float(kappa), float(g), loss.ptr(), opt(al),
                                      opt(dl), opt(hi), opt(lo), work.ptr(), st))
    torch.cuda.synchronize()
    work.read()
    return dict(loss=loss.read().view(np.float32),
                align=None if al is None else al.read().reshape(B, T),
                dlogits=None if dl is None else dl.read().view(np.float32).reshape(B, Tpad, V),
                hi=None if hi is None else hi.read().view(np.uint16).reshape(B, Tpad, V),
                lo=None if lo is None else lo.read().view(np.uint16).reshape(B, Tpad, V))


def same_f32(dev, ref):
    """Bit equality of two float32 arrays, NaN matching NaN."""
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(dev), nan) and np.array_equal(dev.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


def check(logits, labels, T=None, frames=None, kappa=1.0, g=1.0):
    """Device vs align_ref on everything: align and dlogits exactly, loss to LOSS_RTOL, planes = bf16(dlogits) with a zero lo."""
    ref = AR.align_margin(logits, labels, BLANK, kappa, g, frames, T)
    dev = run(logits, labels, T, frames, kappa, g)
    assert np.array_equal(dev["align"], ref["align"]), np.argwhere(dev["align"] != ref["align"])[:8]
    assert same_f32(dev["dlogits"], ref["dlogits"]), "dlogits"
    for b in range(logits.shape[0]):
        print(f"clip {b}: loss device {float(dev['loss'][b])!r} reference {float(ref['loss'][b])!r}")
        if np.isinf(ref["loss"][b]):
            assert np.isinf(dev["loss"][b]) and dev["loss"][b] > 0
        else:
            assert abs(float(dev["loss"][b]) - ref["loss"][b]) <= LOSS_RTOL * abs(ref["loss"][b]), b
    nan = np.isnan(ref["dlogits"])
    hi_f = (dev["hi"].astype(np.uint32) << 16).view(np.float32)
    assert np.isnan(hi_f[nan]).all()
    assert np.array_equal(dev["hi"][~nan], AR.bf16_bits(ref["dlogits"])[~nan]), "hi plane"
    assert (dev["lo"][~nan] == 0).all(), "lo plane"
    return ref, dev


def draw_labels(rng, B, S_max, V, lens, repeats=False, scatter=False):
    """(B, S_max) rows with lens[b] valid ids in [1, V) (blank is 0); scatter: negative padding between the valid ids."""
    lab = np.full((B, S_max), -1, dtype=np.int32)
    for b, n in enumerate(lens):
        ids = rng.integers(1, V, n)
        if repeats and n >= 2:
            ids[1::2] = ids[0:-1:2][: len(ids[1::2])]          # every second id repeats its predecessor
        pos = np.sort(rng.choice(S_max, n, replace=False)) if scatter else np.arange(n)
        lab[b, pos] = ids
    return lab


def draw_logits(rng, B, T, V):
    return (rng.standard_normal((B, T, V)) * 2).astype(np.float32)


# (B, T, V, S_max, label lengths): the smallest case; 63 and 65 states (the first lane boundary of the DPP shift, one and two
# states per lane); one S_max per further states-per-lane variant (4, 6, 8, 16), the last with the back-pointer table staged in
# three blocks; table lengths around one block (512 frames + row 0)
SHAPES = [
    (2, 7, 5, 2, [2, 1]),
    (2, 80, 32, 31, [31, 17]),
    (2, 80, 32, 32, [32, 5]),
    (2, 230, 32, 100, [100, 64]),
    (2, 330, 32, 150, [150, 129]),
    (2, 470, 32, 220, [220, 193]),
    (3, 1499, 32, 450, [450, 300, 7]),
    (2, 512, 8, 5, [5, 3]),
    (2, 513, 8, 5, [5, 3]),
    (2, 514, 8, 5, [5, 3]),
    (1, 1025, 8, 5, [5]),
]


@pytest.mark.parametrize("B,T,V,S_max,lens", SHAPES, ids=[f"B{s[0]}-T{s[1]}-V{s[2]}-S{s[3]}" for s in SHAPES])
def test_shapes_match_the_reference(B, T, V, S_max, lens):
    rng = np.random.default_rng(1000 * S_max + T)
    ref, _ = check(draw_logits(rng, B, T, V), draw_labels(rng, B, S_max, V, lens, repeats=S_max > 2))
    assert np.isfinite(ref["loss"]).all() and (ref["loss"] > 0).all()


def test_vocabulary_not_a_multiple_of_32_and_64_plus():
    rng = np.random.default_rng(33)
    for V in (33, 70):
        check(draw_logits(rng, 2, 40, V), draw_labels(rng, 2, 9, V, [9, 4]))


@pytest.mark.parametrize("g", [1.0, -1.0])
def test_pad_rows_are_zeroed_and_not_read(g):
    rng = np.random.default_rng(7)
    B, T, Tpad, V = 2, 21, 29, 32
    logits = draw_logits(rng, B, Tpad, V)
    logits[:, T:] = np.nan
    ref, dev = check(logits, draw_labels(rng, B, 6, V, [6, 2]), T=T, g=g)
    assert (dev["dlogits"][:, T:].view(np.uint32) == 0).all() and (dev["hi"][:, T:] == 0).all() and (dev["lo"][:, T:] == 0).all()
    assert set(np.unique(dev["dlogits"][:, :T])) <= {-1.0, 0.0, 1.0} and (dev["dlogits"] == g).any()


def test_frames_per_clip_and_infeasible_neighbours():
    """Clip 1 runs at its minimum feasible frame count (S + repeats), clip 2 one below it: +inf and NaN rows.  The neighbours' bits
    equal their solo run at T = T_b."""
    rng = np.random.default_rng(11)
    B, T, V, S_max = 4, 30, 32, 8
    labels = np.full((B, S_max), -1, dtype=np.int32)
    labels[0, :5] = [3, 4, 4, 9, 2]
    labels[1, :6] = [5, 5, 6, 7, 7, 7]          # 6 labels, 3 repeats: 9 frames at least
    labels[2, :6] = [5, 5, 6, 7, 7, 7]
    labels[3, :2] = [8, 1]
    frames = [30, 9, 8, 17]
    logits = draw_logits(rng, B, T, V)
    ref, dev = check(logits, labels, frames=frames)
    assert np.isinf(ref["loss"][2]) and np.isfinite(ref["loss"][[0, 1, 3]]).all()
    assert np.isnan(dev["dlogits"][2, :8]).all() and (dev["dlogits"][2, 8:].view(np.uint32) == 0).all()
    assert (dev["align"][2] == BLANK).all()
    for b in (0, 1, 3):
        tb = frames[b]
        solo = run(logits[b:b + 1, :tb], labels[b:b + 1])
        assert solo["loss"].view(np.uint32)[0] == dev["loss"].view(np.uint32)[b], b
        assert np.array_equal(solo["align"][0], dev["align"][b, :tb]) and (dev["align"][b, tb:] == BLANK).all(), b
        assert np.array_equal(solo["dlogits"][0].view(np.uint32), dev["dlogits"][b, :tb].view(np.uint32)), b
        assert (dev["dlogits"][b, tb:].view(np.uint32) == 0).all(), b


def test_negative_padding_between_valid_ids():
    rng = np.random.default_rng(13)
    B, T, V, S_max = 3, 50, 32, 40
    scattered = draw_labels(rng, B, S_max, V, [12, 30, 1], scatter=True)
    assert (scattered[:, 0] < 0).any() or (np.diff((scattered >= 0).astype(int), axis=1) > 0).any()
    logits = draw_logits(rng, B, T, V)
    _, dev = check(logits, scattered)
    packed = np.full_like(scattered, -1)
    for b in range(B):
        v = scattered[b][scattered[b] >= 0]
        packed[b, :len(v)] = v
    again = run(logits, packed)
    assert np.array_equal(again["align"], dev["align"]) and np.array_equal(again["loss"].view(np.uint32), dev["loss"].view(np.uint32))


def test_repeated_labels_like_the_unk_targets():
    """Lower-cased '<unk>'-style strings: the same characters over and over, with doubled letters."""
    rng = np.random.default_rng(17)
    word = [11, 12, 13, 14, 15, 4]                       # one id per character of a short word and the separator
    row = np.asarray((word * 5)[:-1] + [7, 7, 7], dtype=np.int32)
    labels = np.full((2, 40), -1, dtype=np.int32)
    labels[0, :len(row)] = row
    labels[1, :4] = [9, 9, 9, 9]
    check(draw_logits(rng, 2, 90, 32), labels)


def test_empty_label_row_is_all_blank():
    rng = np.random.default_rng(19)
    labels = np.full((2, 3), -1, dtype=np.int32)
    labels[1, 1] = 2
    ref, dev = check(draw_logits(rng, 2, 12, 8), labels)
    assert (dev["align"][0] == BLANK).all()


def test_hand_example_and_exact_ties():
    """All-zero logits, T = 5, labels (a, a): pi = a 0 a 0 0 by the tie rule alone.  Then logits on a grid of 0.5, whose sums are
    exact in float64: every tie is a true tie."""
    labels = np.asarray([[1, 1]], dtype=np.int32)
    ref, dev = check(np.zeros((1, 5, 4), dtype=np.float32), labels)
    assert dev["align"].tolist() == [[1, 0, 1, 0, 0]]
    rng = np.random.default_rng(23)
    for B, T, V, S_max, lens in [(3, 40, 6, 9, [9, 5, 0]), (2, 200, 4, 70, [70, 33])]:
        grid = (rng.integers(-2, 3, (B, T, V)) * 0.5).astype(np.float32)
        check(grid, draw_labels(rng, B, S_max, V, lens, repeats=True), kappa=0.5)
        check(np.zeros((B, T, V), dtype=np.float32), draw_labels(rng, B, S_max, V, lens, repeats=True), kappa=0.0)


def test_null_outputs_and_repeatability():
    rng = np.random.default_rng(29)
    logits, labels = draw_logits(rng, 2, 33, 32), draw_labels(rng, 2, 10, 32, [10, 3])
    full = run(logits, labels)
    twice = run(logits, labels, calls=2)
    for k in ("loss", "dlogits"):
        assert np.array_equal(full[k].view(np.uint32), twice[k].view(np.uint32)), k
    assert np.array_equal(full["align"], twice["align"]) and np.array_equal(full["hi"], twice["hi"])
    aligner = run(logits, labels, want_dl=False)                        # dlogits NULL: forced aligner + loss only
    assert np.array_equal(aligner["align"], full["align"]) and np.array_equal(aligner["loss"].view(np.uint32), full["loss"].view(np.uint32))
    no_align = run(logits, labels, want_align=False, want_planes=False)
    assert np.array_equal(no_align["dlogits"].view(np.uint32), full["dlogits"].view(np.uint32))
    assert np.array_equal(no_align["loss"].view(np.uint32), full["loss"].view(np.uint32))


def test_python_shims():
    from paa_amd.core import alignment
    rng = np.random.default_rng(31)
    logits, labels = draw_logits(rng, 3, 25, 32), draw_labels(rng, 3, 6, 32, [6, 2, 4])
    frames = [25, 25, 11]
    ref = AR.align_margin(logits, labels, BLANK, 1.5, 1.0, frames)
    z = torch.from_numpy(logits).cuda()
    ids = alignment.forced_alignment(z, torch.from_numpy(labels), frames)
    assert ids.dtype == torch.int16 and np.array_equal(ids.cpu().numpy(), ref["align"])
    loss, dl = alignment.margin_loss(z, labels, 1.5, frames, grad=True)
    assert np.allclose(loss.cpu().numpy(), ref["loss"], rtol=LOSS_RTOL, atol=0) and same_f32(dl.cpu().numpy(), ref["dlogits"])
    assert torch.equal(alignment.margin_loss(z, labels, 1.5, frames), loss)


def test_argument_refusals():
    L = _lib.lib()
    d = C.c_void_p(1 << 20)        # never dereferenced: the arguments are refused first
    ARG, SIZE = _lib.PAA_ERR_ARG, _lib.PAA_ERR_SIZE
    call = lambda logits=d, labels=d, B=2, T=7, Tpad=7, V=5, S=2, blank=0, kappa=1.0, loss=d, dl=d, hi=None, lo=None, work=d: \
        L.paa_align_margin(logits, labels, None, B, T, Tpad, V, S, blank, kappa, 1.0, loss, None, dl, hi, lo, work, None)
    assert call(logits=None) == ARG and call(labels=None) == ARG and call(loss=None) == ARG and call(work=None) == ARG
    assert call(dl=None, hi=d) == ARG and call(lo=d) == ARG                     # planes need dlogits and a hi plane
    assert call(kappa=-0.5) == ARG and call(kappa=float("inf")) == ARG and call(kappa=float("nan")) == ARG
    assert call(work=C.c_void_p((1 << 20) + 8)) == ARG
    assert call(S=512) == SIZE and call(S=0) == SIZE                            # 2 S_max + 1 <= 1024
    assert call(Tpad=6) == SIZE and call(T=0) == SIZE and call(B=0) == SIZE and call(V=1) == SIZE and call(V=257) == SIZE
    assert call(blank=5) == SIZE and call(blank=-1) == SIZE
    assert call(S=512) == SIZE and b"S_max" in L.paa_last_error()
    assert L.paa_align_margin_work_floats(2, 7, 5, 2) > 0
    assert L.paa_model_set_loss(None, 1, 1.0) == ARG
