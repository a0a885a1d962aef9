"""The row kernels (k_ln_fwd, k_ln_bwd, k_softmax_fwd / bwd, the CTC family, k_mul_gelu_grad) on every path the model takes through
them — bf16 planes (hi, hi + lo, interleaved), null f32 outputs, aliased and added operands, score matrices in padded slots, padded CTC
frames with planes and a gradient sign — against the float64 statements of tests/rows_ref.py.

Bounds.  Norm-wise (max |err| / max |ref|) the project's own: 1e-5 LayerNorm / softmax forward, 2e-5 backward, CTC nll 2e-6 and
gradient 1e-5.  Per row (and per element where stated) the kernel is allowed 4 x the error torch float32 makes on the CPU on the same
inputs against the same float64 reference, with a floor of 4 float32 ulps (4 * 2^-23) of the row's largest output: both sum in float32
in different orders; a wrong divisor or a missing eps is two orders above that on the ordinary rows.

Every output lives between two guard blocks of a sentinel bit pattern that must survive; planes written next to an f32 result must be
the planes of THAT result bit for bit; every launch is repeated and must reproduce its bits."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rows_ref as R
from gpu_util import rel_err
from paa_amd import _lib

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23
SENT = {torch.int32: -0x21524111, torch.int16: 0x5EAD}       # 0xDEADBEEF as float32: -6.26e18; 0x5EAD as bf16: 6.2e18


class Guarded:
    """A device tensor with a guard block of the sentinel pattern in front of it and behind it."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(shape))
        self.g = -(-max(shape[-1], 256) // 64) * 64           # at least one row, a multiple of 64 elements (keeps 16-byte alignment)
        self.idt = torch.int32 if dtype == torch.float32 else torch.int16
        self.full = torch.full((self.n + 2 * self.g,), SENT[self.idt], dtype=self.idt, device="cuda")
        self.t = self.full[self.g:self.g + self.n].view(dtype).view(shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).to(dtype))

    @property
    def ptr(self):
        return _lib.ptr(self.t)

    def check(self):
        s = SENT[self.idt]
        assert bool((self.full[:self.g] == s).all()) and bool((self.full[self.g + self.n:] == s).all()), "guard block overwritten"

    def numpy(self):
        a = self.t.cpu().numpy()
        return a.view(np.uint16) if self.idt == torch.int16 else a


class Planes:
    """bf16 planes of a tensor of `shape`: mode None (no planes), "hi", "hi+lo" or "il" (one array, last axis doubled)."""

    def __init__(self, shape, mode):
        self.mode, self.hi, self.lo = mode, None, None
        if mode == "il":
            self.hi = Guarded(tuple(shape[:-1]) + (2 * shape[-1],), torch.int16)
        elif mode:
            self.hi = Guarded(shape, torch.int16)
            self.lo = Guarded(shape, torch.int16) if mode == "hi+lo" else None

    def args(self):
        return (self.hi.ptr if self.hi else None, self.lo.ptr if self.lo else None, int(self.mode == "il"))

    def check(self):
        for p in (self.hi, self.lo):
            if p:
                p.check()

    def bits(self):
        return tuple(None if p is None else p.numpy() for p in (self.hi, self.lo))


def same_bits(a, b):
    """bit equality of two arrays (NaN == NaN, -0 != +0), or of two tuples of optional arrays"""
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_planes_of(pl: Planes, v32):
    """the planes a launch wrote next to its f32 result v32 are the planes of that result, bit for bit"""
    if pl.mode:
        assert same_bits(pl.bits(), R.planes_of(v32, pl.mode)), f"{pl.mode} planes differ from the planes of the f32 result"
    pl.check()


def row_err(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max(-1)


def row_bound(ref, t32, ref_t=None, scale=None):
    """4 x the per-row error of the torch float32 result t32 (against ref_t, default ref), floor 4 ulp of the row's largest output
    (or of `scale`, per row, where given)"""
    et = row_err(t32, ref if ref_t is None else ref_t)
    return np.maximum(4.0 * et, 4.0 * U23 * (np.abs(ref).max(-1) if scale is None else scale))


def over(err, bound):
    """err / bound per row (0 where there is no error at all, a zero bound included)"""
    return np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))


def sync():
    torch.cuda.synchronize()


# ================================================================================ LayerNorm ===
LN_SHAPES = [(1, 4), (5, 32), (7, 252), (130, 768), (9, 1024), (6, 1028), (3, 1280)]
ORD, CONST, OFFS = 0, 1, 2


def ln_variants(rows):
    return ["mixed"] if rows >= 3 else ["ordinary", "const", "offset"]


def ln_inputs(rows, cols, variant, seed):
    """x rows of N(0.3, 2); a constant row (1.5: every partial sum is exact, so variance 0 and y = b exactly); a row of
    100 + 0.01 N(0, 1) (a one-pass variance loses it).  kind[r] says which."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=gen) * 2 + 0.3
    kind = np.full(rows, ORD)
    if variant == "mixed":
        kind[1], kind[rows - 1] = CONST, OFFS
    elif variant != "ordinary":
        kind[:] = CONST if variant == "const" else OFFS
    for r in range(rows):
        if kind[r] == CONST:
            x[r] = 1.5
        elif kind[r] == OFFS:
            x[r] = 100 + 0.01 * torch.randn(cols, generator=gen)
    g = torch.randn(cols, generator=gen) * 0.1 + 1
    b = torch.randn(cols, generator=gen) * 0.1
    dy = torch.randn(rows, cols, generator=gen)
    add = torch.randn(rows, cols, generator=gen)
    return x, g, b, dy, add, kind


def ln_modes(cols):
    return [None, "hi", "hi+lo"] + (["il"] if cols % 32 == 0 else [])


class LnFwd:
    def __init__(self, x, g, b, mode, y=True, stats=True, act=True, yact=True):
        rows, cols = x.shape
        self.y = Guarded((rows, cols)) if y else None
        self.st = Guarded((rows, 2)) if stats else None
        self.yb = Planes((rows, cols), mode)
        self.actb = Planes((rows, cols), mode if act else None)
        self.yact = Guarded((rows, cols)) if yact else None
        _lib.check(_lib.lib().paa_layernorm_fwd_planes(
            _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), self.y.ptr if y else None, self.st.ptr if stats else None, *self.yb.args(),
            *self.actb.args(), self.yact.ptr if yact else None, rows, cols, 1e-5, _lib.stream_ptr()))
        sync()
        for o in (self.y, self.st, self.yb, self.actb, self.yact):
            if o:
                o.check()

    def outs(self):
        return tuple(o.numpy() if o else None for o in (self.y, self.st, self.yact)) + self.yb.bits() + self.actb.bits()


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_fwd(rows, cols):
    for vi, variant in enumerate(ln_variants(rows)):
        x, g, b, _, _, kind = ln_inputs(rows, cols, variant, 10 + vi)
        yr, ar, sr = R.ln_fwd(x, g, b, 1e-5)
        yt = F.layer_norm(x, (cols,), g, b, eps=1e-5)
        at = F.gelu(yt)
        xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
        ordi = kind == ORD
        first = None
        for mode in ln_modes(cols):
            A = LnFwd(xd, gd, bd, mode)
            y, st, ya = A.y.numpy(), A.st.numpy(), A.yact.numpy()
            # statistics: every element passes through at most 13 float32 additions (2 inside its float4, <= 5 per lane, 6 in the
            # wave reduction) and one division, so |mean err| <= 14 u mean|x| (u = 2^-24) whatever the order; 16 u allowed.  rstd:
            # the same bound on the variance halves under the square root, plus the 2 ulp of rsqrtf; 16 u relative allowed.
            em = np.abs(st[:, 0] - sr[:, 0]) / np.abs(x.double().numpy()).mean(-1)
            es = np.abs(st[:, 1] / sr[:, 1] - 1)
            # y against float64; gelu(y) against the float64 GELU of the y THIS launch wrote (torch: of the y torch wrote): the error y
            # carries is bounded by the check on y, and on the 100 +- 0.01 row it is a thousand times the error of the GELU itself
            ey = over(row_err(y, yr), row_bound(yr, yt.numpy()))
            ea = over(row_err(ya, R.gelu(y)), row_bound(ar, at.numpy(), R.gelu(yt)))
            print(f"ln fwd {rows}x{cols} {variant} {mode}: mean {em.max() / U23 * 2:.2f} u rstd {es.max() / U23 * 2:.2f} u; "
                  f"y / bound {ey.max():.3f} gelu / bound {ea.max():.3f}; offset rows y err "
                  f"{rel_err(y[kind == OFFS], yr[kind == OFFS]) if (kind == OFFS).any() else 0:.2e} "
                  f"(torch {rel_err(yt.numpy()[kind == OFFS], yr[kind == OFFS]) if (kind == OFFS).any() else 0:.2e})")
            assert em.max() <= 16 * U23 / 2 and es.max() <= 16 * U23 / 2          # measured: mean <= 0.99 u, rstd <= 4.4 u
            # measured: ordinary rows <= 0.36 of the bound; 100 +- 0.01 rows 5.8e-8 .. 4.9e-4 norm-wise where torch has 8.1e-5 .. 3.2e-4
            # (0.71 of the bound at most)
            assert (ey <= 1).all(), ("y rows over 4 x torch float32", np.nonzero(ey > 1)[0], ey.max())
            assert (ea <= 1).all(), ("gelu(y) rows over 4 x torch float32", np.nonzero(ea > 1)[0], ea.max())      # measured <= 0.16
            if ordi.any():
                e1, e2 = rel_err(y[ordi], yr[ordi]), rel_err(ya[ordi], ar[ordi])
                print(f"    ordinary rows norm-wise: y {e1:.2e} gelu {e2:.2e}")
                assert e1 < 1e-5 and e2 < 1e-5                # measured 8.3e-8 .. 1.6e-7 and 5.3e-8 .. 1.5e-7
            assert np.array_equal(y[kind == CONST], np.broadcast_to(b.numpy(), y.shape)[kind == CONST])     # variance 0: y = b
            assert_planes_of(A.yb, y)
            assert_planes_of(A.actb, ya)
            assert same_bits(LnFwd(xd, gd, bd, mode).outs(), A.outs())                         # reproducible
            if first is None:
                first = A
                # neither the GELU outputs nor the statistics change y
                assert same_bits(LnFwd(xd, gd, bd, None, act=False, yact=False).y.numpy(), y)
                assert same_bits(LnFwd(xd, gd, bd, None, stats=False, yact=False).y.numpy(), y)
            else:
                assert same_bits((y, st, ya), first.outs()[:3])                                # the planes do not change the f32 results
                # planes only, as the encoder calls it: the same planes as next to the f32 results
                N = LnFwd(xd, gd, bd, mode, y=False, yact=False)
                assert same_bits(N.yb.bits() + N.actb.bits(), A.yb.bits() + A.actb.bits()) and same_bits(N.st.numpy(), st)
                N = LnFwd(xd, gd, bd, mode, y=False, act=False, yact=False)
                assert same_bits(N.yb.bits(), A.yb.bits())


class LnBwd:
    def __init__(self, dy, x, g, st, add, mode, dx="own"):
        """dx: "own" buffer, "alias" (in place on a guarded copy of dy) or None"""
        rows, cols = x.shape
        self.dy = Guarded((rows, cols), init=dy.cpu().numpy())
        self.dx = Guarded((rows, cols)) if dx == "own" else self.dy if dx == "alias" else None
        self.dxb = Planes((rows, cols), mode)
        _lib.check(_lib.lib().paa_layernorm_bwd_planes(
            self.dy.ptr, _lib.ptr(x), _lib.ptr(g), _lib.ptr(st), _lib.ptr(add), self.dx.ptr if self.dx else None, *self.dxb.args(),
            rows, cols, _lib.stream_ptr()))
        sync()
        self.dy.check()
        self.dxb.check()
        if self.dx:
            self.dx.check()
        if dx != "alias":
            assert same_bits(self.dy.numpy(), dy.cpu().numpy()), "dy was modified"


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_bwd(rows, cols):
    for vi, variant in enumerate(ln_variants(rows)):
        x, g, b, dy, add, kind = ln_inputs(rows, cols, variant, 20 + vi)
        sr = R.ln_stats(x, 1e-5)
        st32 = sr.astype(np.float32)                # the kernel's statistics: the float64 ones rounded, not a forward kernel's
        xt = x.clone().requires_grad_(True)
        F.layer_norm(xt, (cols,), g, b, eps=1e-5).backward(dy)
        xd, gd, dyd, std, addd = x.cuda(), g.cuda(), dy.cuda(), torch.from_numpy(st32).cuda(), add.cuda()
        ordi = kind == ORD
        for with_add in (False, True):
            ref = R.ln_bwd(dy, x, g, st32, add if with_add else None)         # the same function of the same rounded statistics
            true = R.ln_bwd(dy, x, g, sr, add if with_add else None)          # what torch float32 approximates
            t32 = (xt.grad + add if with_add else xt.grad).numpy()
            a = addd if with_add else None
            for mode in ln_modes(cols):
                A = LnBwd(dyd, xd, gd, std, a, mode)
                dx = A.dx.numpy()
                e = over(row_err(dx, ref), row_bound(ref, t32, true))              # measured <= 0.23 of the bound
                print(f"ln bwd {rows}x{cols} {variant} add={with_add} {mode}: dx / bound {e.max():.3f}")
                assert (e <= 1).all(), ("dx rows over 4 x torch float32", np.nonzero(e > 1)[0], e.max())
                if ordi.any():
                    e1 = rel_err(dx[ordi], ref[ordi])
                    print(f"    ordinary rows norm-wise: {e1:.2e}")
                    assert e1 < 2e-5                      # measured 1.9e-8 .. 9.1e-8
                assert_planes_of(A.dxb, dx)
                assert same_bits(LnBwd(dyd, xd, gd, std, a, mode).dx.numpy(), dx)                     # reproducible
                I = LnBwd(dyd, xd, gd, std, a, mode, dx="alias")                                      # in place on dy, as the encoder
                assert same_bits(I.dx.numpy(), dx) and same_bits(I.dxb.bits(), A.dxb.bits())
                if mode:
                    N = LnBwd(dyd, xd, gd, std, a, mode, dx=None)                                     # planes only (conv stack)
                    assert same_bits(N.dxb.bits(), A.dxb.bits())


# ================================================================================= softmax ===
SM_SHAPES = [(1, 5, 5, 1, 4), (3, 5, 8, 63, 64), (2, 7, 8, 64, 64), (3, 9, 12, 65, 72), (2, 33, 40, 499, 512)]


def sm_buffer(n_mat, rpm, mld, cols, ld, vals):
    """(n_mat * mld, ld) guarded buffer: valid rows hold vals (n_mat * rpm, cols) and NaN in the pad columns, every pad row the
    sentinel"""
    buf = Guarded((n_mat * mld, ld))
    idx = torch.tensor([m * mld + r for m in range(n_mat) for r in range(rpm)], device="cuda")
    rows = torch.full((n_mat * rpm, ld), float("nan"))
    rows[:, :cols] = vals
    buf.t[idx] = rows.cuda()
    return buf, idx


def sm_read(buf, idx, n_mat, mld, cols):
    """valid rows' valid columns; asserts zero pad columns, untouched pad rows and guards"""
    buf.check()
    pad = torch.ones(n_mat * mld, dtype=torch.bool, device="cuda")
    pad[idx] = False
    assert bool((buf.t.view(torch.int32)[pad] == SENT[torch.int32]).all()), "pad rows between the matrices were written"
    v = buf.t[idx].cpu().numpy()
    assert np.array_equal(v[:, cols:].view(np.int32), np.zeros_like(v[:, cols:], dtype=np.int32)), "pad columns are not +0"
    return v[:, :cols]


def softmax_case(n_mat, rpm, mld, cols, ld, amp, scale, seed):
    gen = torch.Generator().manual_seed(seed)
    s = torch.randn(n_mat * rpm, cols, generator=gen) * amp
    dp = torch.randn(n_mat * rpm, cols, generator=gen)
    pr = R.softmax_fwd(s, scale)
    pt = torch.softmax(s * scale, -1).numpy()
    L = _lib.lib()

    def fwd():
        buf, idx = sm_buffer(n_mat, rpm, mld, cols, ld, s)
        _lib.check(L.paa_softmax_fwd_mats(buf.ptr, n_mat, rpm, mld, cols, ld, scale, _lib.stream_ptr()))
        sync()
        return sm_read(buf, idx, n_mat, mld, cols)
    p = fwd()
    assert same_bits(fwd(), p)
    e1 = rel_err(p, pr)
    er = over(row_err(p, pr), row_bound(pr, pt))
    # per element, relative, wherever float32 still has its full precision (below 1e-30 the hardware exp flushes to zero)
    big = pr >= 1e-30
    rel = np.abs(p - pr)[big] / pr[big]
    rel_t = np.abs(pt - pr)[big] / pr[big]
    eb = max(4 * rel_t.max(), 4 * U23)
    print(f"softmax fwd {(n_mat, rpm, mld, cols, ld)} amp {amp}: norm-wise {e1:.2e}; row / bound {er.max():.3f}; per element "
          f"{rel.max():.2e} (torch {rel_t.max():.2e}, bound {eb:.2e}); smallest p {pr.min():.1e}")
    assert e1 < 1e-5                            # measured 8.3e-8 .. 8.9e-8, wide range 1.3e-7
    assert (er <= 1).all(), ("rows over 4 x torch float32", np.nonzero(er > 1)[0], er.max())      # measured <= 0.38 of the bound
    # measured 2.2e-7 .. 3.8e-7 where torch has 1.9e-7 .. 3.0e-7; wide range 7.3e-6 where torch has 4.0e-6 (arguments down to -69:
    # the rounding of x - max and of its product with log2 e).  __expf needs no allowance of its own.
    assert rel.max() <= eb
    assert (p[~big] >= 0).all() and (p[~big] <= 2e-30).all()

    p32 = pr.astype(np.float32)                     # the backward's P: the float64 reference rounded, not the forward kernel's
    dr = R.softmax_bwd(dp, p32, scale)
    p32t = torch.from_numpy(p32)
    dt = (scale * p32t * (dp - (dp * p32t).sum(-1, keepdim=True))).numpy()
    pbuf, idx = sm_buffer(n_mat, rpm, mld, cols, ld, p32t)

    def bwd():
        buf, idx = sm_buffer(n_mat, rpm, mld, cols, ld, dp)
        _lib.check(L.paa_softmax_bwd_mats(buf.ptr, pbuf.ptr, n_mat, rpm, mld, cols, ld, scale, _lib.stream_ptr()))
        sync()
        return sm_read(buf, idx, n_mat, mld, cols)
    d = bwd()
    assert same_bits(bwd(), d)
    pbuf.check()
    assert same_bits(pbuf.t[idx].cpu().numpy()[:, :cols], p32), "P was modified"
    e2 = rel_err(d, dr)
    # Floor of the row bound: 4 ulp of the row's largest term BEFORE the subtraction, scale P_j (|dP_j| + |dot|), not of its largest
    # output.  dS_j = scale P_j (dP_j - dot) cancels on a nearly one-hot row, and any float32 dot carries about half an ulp of |dot|:
    # on row 13 of the wide-range case (P_max = 0.998, dot = 0.662, largest |dS| 1.7e-4) the kernel's dot is 1 ulp off (5.8e-8) and
    # torch's happens to be 0.03 ulp off (1.6e-9), so neither 4 x torch nor 4 ulp of the largest output (8.3e-11) describes what
    # float32 can do there; 9.0 times that bound was measured.  On ordinary rows the two floors are of the same size.
    dot = np.abs((dp.double().numpy() * p32).sum(-1, keepdims=True))
    term = (scale * p32 * (np.abs(dp.double().numpy()) + dot)).max(-1)
    eb = over(row_err(d, dr), row_bound(dr, dt, scale=term))
    print(f"softmax bwd: norm-wise {e2:.2e}; row / bound {eb.max():.3f}")
    assert e2 < 2e-5                            # measured 5.0e-8 .. 6.3e-8, wide range 2.4e-7
    assert (eb <= 1).all(), ("rows over 4 x torch float32", np.nonzero(eb > 1)[0], eb.max())      # measured <= 0.19 of the bound


@pytest.mark.parametrize("shape", SM_SHAPES)
def test_softmax_mats(shape):
    softmax_case(*shape, amp=3.0, scale=0.125, seed=30)


def test_softmax_mats_wide_range():
    """scores 30 N(0, 1) at scale 1: a dynamic range of about e^-100 per row, which only max subtraction survives"""
    softmax_case(2, 33, 40, 499, 512, amp=30.0, scale=1.0, seed=31)


# ===================================================================================== CTC ===
# (T, V, S_max): recursion kernel and side of the LDS-table switch (8 T V + exchange + labels <= 150 KiB)
CTC_CASES = [(37, 5, 20),        # k_ctc_rec<1> (NS = 1), table in LDS, T V odd (the copy tail), V < 32
             (80, 256, 31),      # k_ctc_rec<1> (NS = 1), table in global memory
             (70, 256, 100),     # k_ctc_rec_mw<4, 1>, table in LDS (152820 bytes of 153600)
             (80, 256, 60),      # k_ctc_rec_mw<2, 1>, table in global memory
             (71, 65, 300),      # k_ctc_rec_mw<16, 2>, table in LDS, T V odd, V = 64 + 1
             (80, 256, 300),     # k_ctc_rec_mw<16, 2>, table in global memory
             (41, 29, 520)]      # k_ctc (2 S_max + 1 > 1024), T V odd
FEASIBLE = np.array([True, True, True, False, True])


def ctc_inputs(T, V, S_max, seed):
    """Five clips: random labels with a repeat; negative labels in the interior of the row; all repeats of one class; an infeasible
    clip; an empty one.  Labels avoid classes 0 and V - 1 (either may be the blank); label lengths <= T / 2."""
    gen = torch.Generator().manual_seed(seed)
    Tpad = T + 3
    logits = torch.randn(5, Tpad, V, generator=gen) * 2
    n = min(S_max, T // 2)
    lab = torch.full((5, S_max), -100, dtype=torch.int64)
    lab[0, :n] = torch.randint(1, V - 1, (n,), generator=gen)
    lab[0, 2] = lab[0, 1]
    lab[1, :n] = torch.randint(1, V - 1, (n,), generator=gen)
    lab[1, 1::7] = -100
    lab[1, 3] = -1
    lab[1, 4] = lab[1, 2]                                        # [c, -100, d, -1, d, ...]: a repeat across two masked entries
    lab[2, :n] = 1 + (seed % (V - 2))
    if 2 * S_max - 1 > T:
        lab[3, :] = 2                                            # S_max repeats need 2 S_max - 1 frames
    else:
        lab[3, :n] = torch.randint(1, V - 1, (n,), generator=gen)
        logits[3, :, int(lab[3, 0])] = -float("inf")             # a class the clip needs is impossible in every frame
    logits[:, T:] = float("nan")                                 # pad frames: must not be read
    return logits, lab, Tpad


class Ctc:
    def __init__(self, lg, lab, T, Tpad, V, S_max, blank, gs, work_fill, lo=True):
        B = lg.shape[0]
        L = _lib.lib()
        self.nll = Guarded((B,))
        self.dl = Guarded((B, Tpad, V))
        self.pl = Planes((B, Tpad, V), "hi+lo" if lo else "hi")
        work = torch.full((L.paa_ctc_work_floats(B, T, V, S_max),), work_fill, device="cuda")
        hi, lo_, _ = self.pl.args()
        _lib.check(L.paa_ctc_padded(_lib.ptr(lg), _lib.ptr(lab), B, T, Tpad, V, S_max, blank, gs, self.nll.ptr, self.dl.ptr, hi, lo_,
                                    _lib.ptr(work), _lib.stream_ptr()))
        sync()
        self.nll.check()
        self.dl.check()
        self.pl.check()

    def outs(self):
        return (self.nll.numpy(), self.dl.numpy()) + self.pl.bits()


@pytest.mark.parametrize("T,V,S_max", CTC_CASES)
def test_ctc_padded(T, V, S_max):
    logits, lab, Tpad = ctc_inputs(T, V, S_max, 40 + T + V)
    lg, labd = logits.cuda(), lab.to(torch.int32).cuda()
    fin = FEASIBLE
    for blank in (0, V - 1):
        nr, gr = R.ctc_padded(logits, lab, T, blank)
        assert np.array_equal(np.isfinite(nr), fin)
        A = Ctc(lg, labd, T, Tpad, V, S_max, blank, 1.0, float("nan"))
        nll, dl, hi, lo = A.outs()
        assert same_bits(Ctc(lg, labd, T, Tpad, V, S_max, blank, 1.0, 0.0).outs(), A.outs())          # reproducible, work not read
        assert np.array_equal(np.isfinite(nll), fin) and nll[3] == np.inf
        e1, e2 = rel_err(nll[fin], nr[fin]), rel_err(dl[fin], gr[fin])
        ec = max(rel_err(dl[b], gr[b]) for b in np.nonzero(fin)[0])
        print(f"ctc T={T} V={V} S_max={S_max} blank={blank}: nll {e1:.2e} grad {e2:.2e} worst clip {ec:.2e}")
        assert e1 < 2e-6 and e2 < 1e-5 and ec < 1e-5                         # measured 1.5e-8 .. 4.9e-8, 2.4e-7 .. 9.2e-7, <= 9.3e-7
        # the infeasible clip: NaN on its T frames, f32 and planes; pad frames exactly +0 everywhere
        assert np.isnan(dl[3, :T]).all() and np.isnan(R.planes_value(hi[3, :T])).all() and np.isnan(R.planes_value(lo[3, :T])).all()
        for a in (dl.view(np.int32), hi, lo):
            assert not a[:, T:].any(), "pad frames are not +0"
        assert same_bits((hi[fin], lo[fin]), R.planes_of(dl[fin], "hi+lo"))
        # direction -1 (targeted): the exact negation, planes included
        M = Ctc(lg, labd, T, Tpad, V, S_max, blank, -1.0, float("nan"))
        nll_m, dl_m, hi_m, lo_m = M.outs()
        assert same_bits(nll_m, nll) and np.array_equal(dl_m[fin], -dl[fin]) and np.isnan(dl_m[3, :T]).all()
        assert np.array_equal(R.planes_value(hi_m[fin]), -R.planes_value(hi[fin]))
        assert np.array_equal(R.planes_value(lo_m[fin]), -R.planes_value(lo[fin]))
        assert same_bits((hi_m[fin], lo_m[fin]), R.planes_of(dl_m[fin], "hi+lo"))
        assert not dl_m[:, T:].view(np.int32).any() and not hi_m[:, T:].any() and not lo_m[:, T:].any()
        # grad_scale 0.5, hi plane only (bf16 mode)
        H = Ctc(lg, labd, T, Tpad, V, S_max, blank, 0.5, float("nan"), lo=False)
        nll_h, dl_h, hi_h, _ = H.outs()
        e3 = rel_err(dl_h[fin], 0.5 * gr[fin])
        print(f"    grad_scale 0.5: grad {e3:.2e}")
        assert same_bits(nll_h, nll) and e3 < 1e-5 and np.isnan(dl_h[3, :T]).all()
        assert same_bits(hi_h[fin], R.planes_of(dl_h[fin], "hi")[0]) and not hi_h[:, T:].any() and not dl_h[:, T:].view(np.int32).any()


# ---- the wave-synchronous recursion as a family: one arithmetic per state whatever the number of states per lane (NS) --------------
# Cases by name -> (logits (B, Tpad, V), labels (B, S_max), T, frames or None).  Without frames a case runs through paa_ctc_padded
# with hi + lo planes, with frames through paa_ctc_len.  tools/ctc_parent_bits.py walks the same dictionary.
CAP_SMAX = [25, 60, 100, 150, 250, 400]            # NS = 1, 2, 4, 6, 8, 16
CAP_T, CAP_V, CAP_FRAMES = 64, 16, [64, 9, 50]
FULL_SMAX = [31, 63, 127, 191, 255, 511]           # 2 S_max + 1 = 64 NS - 1: the last lane's last slots hold live states
FULL_V = 6
WS_BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_rec_parent.json")


def cap_inputs(S_max):
    """Three clips whose label rows do not depend on the capacity: 25 random labels with one repeat; a single label; 25 labels (they
    fit the 50 frames CAP_FRAMES gives that clip).  Padded with -100 to S_max."""
    gen = torch.Generator().manual_seed(60)
    logits = torch.randn(3, CAP_T, CAP_V, generator=gen) * 2
    lab = torch.full((3, S_max), -100, dtype=torch.int64)
    lab[0, :25] = torch.randint(1, CAP_V - 1, (25,), generator=gen)
    lab[0, 6] = lab[0, 5]
    lab[1, 0] = 3
    lab[2, :25] = torch.randint(1, CAP_V - 1, (25,), generator=gen)
    return logits, lab


def full_inputs(S_max):
    """T = 2 S_max + 8 frames, three clips: exactly S_max labels with adjacent repeats at positions 1-2 and at the last two; S_max - 1
    labels; one label.  S_max labels with r repeats need S_max + r <= 2 S_max - 1 frames: every clip is feasible, also in the
    T - 3 frames full_frames gives clip 1."""
    gen = torch.Generator().manual_seed(70 + S_max)
    T = 2 * S_max + 8
    logits = torch.randn(3, T, FULL_V, generator=gen) * 2
    lab = torch.full((3, S_max), -100, dtype=torch.int64)
    lab[0] = torch.randint(1, FULL_V - 1, (S_max,), generator=gen)
    lab[0, 2] = lab[0, 1]
    lab[0, S_max - 1] = lab[0, S_max - 2]
    lab[1, :S_max - 1] = torch.randint(1, FULL_V - 1, (S_max - 1,), generator=gen)
    lab[2, 0] = 2
    return logits, lab, T


def full_frames(T):
    return [T, T - 3, 5]


def ws_cases():
    cases = {}
    for S_max in CAP_SMAX:
        logits, lab = cap_inputs(S_max)
        cases[f"cap{S_max}"] = (logits, lab, CAP_T, None)
        cases[f"cap{S_max}_len"] = (logits, lab, CAP_T, CAP_FRAMES)
    for S_max in FULL_SMAX:
        logits, lab, T = full_inputs(S_max)
        cases[f"full{S_max}"] = (logits, lab, T, None)
        cases[f"full{S_max}_len"] = (logits, lab, T, full_frames(T))
    for T, V, S_max in CTC_CASES[:6]:
        logits, lab, _ = ctc_inputs(T, V, S_max, 40 + T + V)
        cases[f"rows{T}x{V}x{S_max}"] = (logits, lab, T, None)
    return cases


_ws_cases, _ws_runs = {}, {}


def ws_case(name):
    if not _ws_cases:
        _ws_cases.update(ws_cases())
    return _ws_cases[name]


def ws_run(name, blank):
    """(nll, dlogits, hi, lo) of a case on the GPU, computed once per session; hi and lo are None for the paa_ctc_len cases"""
    if (name, blank) in _ws_runs:
        return _ws_runs[name, blank]
    logits, lab, T, frames = ws_case(name)
    B, Tpad, V = logits.shape
    S_max = lab.shape[1]
    lg, labd = logits.cuda(), lab.to(torch.int32).cuda()
    if frames is None:
        out = Ctc(lg, labd, T, Tpad, V, S_max, blank, 1.0, float("nan")).outs()
    else:
        L = _lib.lib()
        nll, dl = Guarded((B,)), Guarded((B, T, V))
        work = torch.full((L.paa_ctc_work_floats(B, T, V, S_max),), float("nan"), device="cuda")
        fr = torch.tensor(frames, dtype=torch.int32, device="cuda")
        _lib.check(L.paa_ctc_len(_lib.ptr(lg), _lib.ptr(labd), _lib.ptr(fr), B, T, V, S_max, blank, 1.0, nll.ptr, dl.ptr,
                                 _lib.ptr(work), _lib.stream_ptr()))
        sync()
        nll.check()
        dl.check()
        out = (nll.numpy(), dl.numpy(), None, None)
    _ws_runs[name, blank] = out
    return out


def ws_bits(name, blank):
    """what the fixture keeps of a run: nll as uint32 bit patterns, SHA-256 of the dlogits bytes of the first T frames of every clip"""
    nll, dl = ws_run(name, blank)[:2]
    T = ws_case(name)[2]
    return {"nll": [int(v) for v in nll.view(np.uint32)], "dlogits_sha256": hashlib.sha256(np.ascontiguousarray(dl[:, :T]).tobytes()).hexdigest()}


def ctc_ref_frames(logits, lab, frames, blank):
    """float64 CTC of every clip over its own first frames[b] frames: nll (B), gradient (B, T, V) with zero rows beyond"""
    B, T, V = logits.shape
    nll, g = np.zeros(B), np.zeros((B, T, V))
    for b, tb in enumerate(frames):
        n1, g1 = R.ctc_padded(logits[b:b + 1, :tb], lab[b:b + 1], tb, blank)
        nll[b], g[b, :tb] = n1[0], g1[0]
    return nll, g


def test_ctc_capacity_does_not_change_the_bits():
    """The same label rows padded to six capacities run the recursion at NS = 1, 2, 4, 6, 8, 16 states per lane: nll, dlogits and
    the bf16 planes are bit-equal across all six, with and without per-clip frame counts."""
    for blank in (0, CAP_V - 1):
        for suffix in ("", "_len"):
            first = ws_run(f"cap{CAP_SMAX[0]}{suffix}", blank)
            assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
            if suffix:
                for b, tb in enumerate(CAP_FRAMES):
                    assert not first[1][b, tb:].view(np.int32).any(), "rows beyond the clip's frames are not +0"
            for S_max in CAP_SMAX[1:]:
                out = ws_run(f"cap{S_max}{suffix}", blank)
                for what, a, b in zip(("nll", "dlogits", "hi plane", "lo plane"), first, out):
                    assert same_bits(a, b), f"{what} at S_max={S_max} differs from S_max={CAP_SMAX[0]} (blank {blank}, frames {suffix != ''})"


@pytest.mark.parametrize("S_max", FULL_SMAX)
def test_ctc_full_label_rows(S_max):
    """Label rows that fill the capacity (2 S_max + 1 = 64 NS - 1 states: every lane and every slot live) against float64"""
    logits, lab, T = full_inputs(S_max)
    for blank in (0, FULL_V - 1):
        for frames in (None, full_frames(T)):
            nr, gr = R.ctc_padded(logits, lab, T, blank) if frames is None else ctc_ref_frames(logits, lab, frames, blank)
            assert np.isfinite(nr).all() and np.isfinite(gr).all()
            nll, dl = ws_run(f"full{S_max}" + ("" if frames is None else "_len"), blank)[:2]
            assert np.isfinite(nll).all()
            e1, e2 = rel_err(nll, nr), rel_err(dl, gr)
            ec = max(rel_err(dl[b], gr[b]) for b in range(3))
            print(f"ctc full rows S_max={S_max} T={T} blank={blank} frames={frames}: nll {e1:.2e} grad {e2:.2e} worst clip {ec:.2e}")
            assert e1 < 2e-6 and e2 < 1e-5 and ec < 1e-5
            if frames is not None:
                for b, tb in enumerate(frames):
                    assert not dl[b, tb:].view(np.int32).any(), "rows beyond the clip's frames are not +0"


def test_ctc_bits_of_the_parent():
    """nll and dlogits of every case above and of the wave-synchronous CTC_CASES are, bit for bit, what the commit named in the
    fixture computed (tools/ctc_parent_bits.py wrote it from a build of that commit): merging the recursion kernels changed no bit."""
    with open(WS_BITS) as f:
        gold = json.load(f)
    names = list(ws_cases())
    assert sorted(gold["cases"]) == sorted(names)
    for name in names:
        V = ws_case(name)[0].shape[2]
        assert sorted(gold["cases"][name]) == sorted([str(0), str(V - 1)])
        for blank in (0, V - 1):
            got, want = ws_bits(name, blank), gold["cases"][name][str(blank)]
            if got["nll"] != want["nll"]:
                b = next(i for i, (x, y) in enumerate(zip(got["nll"], want["nll"])) if x != y)
                raise AssertionError(f"{name}, blank {blank}: nll of clip {b} is {got['nll'][b]:#010x}, {gold['commit']} gave {want['nll'][b]:#010x}")
            assert got["dlogits_sha256"] == want["dlogits_sha256"], f"{name}, blank {blank}: dlogits differ from those of {gold['commit']}"


# =============================================================================== GELU grad ===
SPECIAL = [1.0, -1.0, 0.0, 1e-3, -1e-3, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0]


@pytest.mark.parametrize("n", [1, 255, 4096 * 256 + 77, 4096])
def test_mul_gelu_grad(n):
    """n = 4096 * 256 + 77 loops the grid; n = 4096 is there for the interleaved planes (n % 32 == 0)"""
    gen = torch.Generator().manual_seed(50)
    pre = torch.randn(n, generator=gen) * 2
    k = min(n, len(SPECIAL))
    pre[:k] = torch.tensor(SPECIAL[:k])
    pre[n - k:] = torch.tensor(SPECIAL[:k])              # the last elements belong to the second trip of the grid-stride loop
    dy = torch.randn(n, generator=gen)
    gr = R.gelu_grad(pre)
    ref = dy.double().numpy() * gr
    pt = pre.clone().requires_grad_(True)
    F.gelu(pt).sum().backward()
    et = np.abs(pt.grad.double().numpy() - gr).max()
    # per element: 4 x the largest error torch float32 makes on gelu' over these inputs (floor 4 ulp of 1; |gelu'| <= 1.13), times
    # |dy|.  Absolute, not relative: 0.5 (1 + erf) cancels to an absolute 6e-8 for x <= -5 in any float32 evaluation.
    bound = 4 * max(et, U23) * np.abs(dy.double().numpy()) + 1e-45
    dyd, pred = dy.cuda(), pre.cuda()
    L = _lib.lib()

    def run(f32, mode):
        out = Guarded((n,)) if f32 else None
        pl = Planes((n,), mode)
        _lib.check(L.paa_mul_gelu_grad_planes(_lib.ptr(dyd), _lib.ptr(pred), out.ptr if f32 else None, *pl.args(), n, _lib.stream_ptr()))
        sync()
        if f32:
            out.check()
        pl.check()
        return (out.numpy() if f32 else None), pl
    v, _ = run(True, None)
    e = np.abs(v - ref) / bound                              # measured <= 0.20 of the bound; |err| / |dy| <= 1.9e-7
    print(f"mul_gelu_grad n={n}: err / bound {e.max():.3f} (torch float32 gelu' error {et:.2e}); largest |err| / |dy| "
          f"{(np.abs(v - ref) / np.abs(dy.double().numpy())).max():.2e}")
    assert np.isfinite(v).all() and (e <= 1).all(), (np.nonzero(e > 1)[0][:8], e.max())
    assert same_bits(run(True, None)[0], v)
    for mode in ["hi", "hi+lo"] + (["il"] if n % 32 == 0 else []):
        v2, pl = run(True, mode)                            # both
        assert same_bits(v2, v)
        assert_planes_of(pl, v2)
        _, pn = run(False, mode)                            # planes only, as the positional convolution's backward
        assert same_bits(pn.bits(), pl.bits())
    if n % 32:
        hi = Guarded((2 * n,), torch.int16)
        assert L.paa_mul_gelu_grad_planes(_lib.ptr(dyd), _lib.ptr(pred), None, hi.ptr, None, 1, n, _lib.stream_ptr()) == _lib.PAA_ERR_ARG
        sync()
        assert not (hi.t != SENT[torch.int16]).any()


def test_interleaved_planes_refused_on_ragged_rows():
    """il planes of rows that are no multiple of 32 elements are unsupported by design: refused, nothing launched"""
    L = _lib.lib()
    x = torch.zeros(2, 252, device="cuda")
    g = torch.ones(252, device="cuda")
    hi = Guarded((2, 504), torch.int16)
    st = torch.zeros(2, 2, device="cuda")
    assert L.paa_layernorm_fwd_planes(_lib.ptr(x), _lib.ptr(g), _lib.ptr(g), None, _lib.ptr(st), hi.ptr, None, 1, None, None, 0, None,
                                      2, 252, 1e-5, _lib.stream_ptr()) == _lib.PAA_ERR_ARG
    assert L.paa_layernorm_bwd_planes(_lib.ptr(x), _lib.ptr(x), _lib.ptr(g), _lib.ptr(st), None, None, hi.ptr, None, 1, 2, 252,
                                      _lib.stream_ptr()) == _lib.PAA_ERR_ARG
    sync()
    assert not (hi.t != SENT[torch.int16]).any()
    hi.check()
