"""No-GPU checks of tests/rows_ref.py (the float64 references test_gpu_rows.py compares the row kernels with) against torch
float64 autograd, of the bf16 plane helpers, and of the argument refusals of the row-kernel test entries that return before
any HIP call."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rows_ref as R
from paa_amd.model import bf16_to_f32, interleave_planes, split_bf16


def _err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.mark.parametrize("rows,cols", [(3, 4), (5, 36), (4, 1028)])
def test_layernorm_reference_matches_autograd(rows, cols):
    torch.manual_seed(0)
    x = (torch.randn(rows, cols, dtype=torch.float64) * 2 + 0.3).requires_grad_(True)
    g = torch.randn(cols, dtype=torch.float64) * 0.1 + 1
    b = torch.randn(cols, dtype=torch.float64) * 0.1
    dy, add = torch.randn(rows, cols, dtype=torch.float64), torch.randn(rows, cols, dtype=torch.float64)
    y = F.layer_norm(x, (cols,), g, b, eps=1e-5)
    a = F.gelu(y)
    y.backward(dy)
    yr, ar, st = R.ln_fwd(x.detach(), g, b, 1e-5)
    assert _err(yr, y.detach()) <= 1e-12 and _err(ar, a.detach()) <= 1e-12
    xd = x.detach()
    assert _err(st[:, 0], xd.mean(-1)) <= 1e-12
    assert _err(st[:, 1], 1 / torch.sqrt(xd.var(-1, unbiased=False) + 1e-5)) <= 1e-12
    assert _err(R.ln_bwd(dy, xd, g, st), x.grad) <= 1e-12
    assert _err(R.ln_bwd(dy, xd, g, st, add), x.grad + add) <= 1e-12


def test_layernorm_reference_constant_row():
    x = np.full((2, 8), 1.5)
    b = np.arange(8.0)
    y, a, st = R.ln_fwd(x, np.ones(8), b, 1e-5)
    assert np.array_equal(y, np.stack([b, b])) and np.array_equal(st[:, 0], [1.5, 1.5])
    assert _err(st[:, 1], 1e-5 ** -0.5) <= 1e-9


@pytest.mark.parametrize("scale,amp", [(0.125, 3.0), (1.0, 30.0)])
def test_softmax_reference_matches_autograd(scale, amp):
    torch.manual_seed(1)
    s = (torch.randn(7, 65, dtype=torch.float64) * amp).requires_grad_(True)
    dp = torch.randn(7, 65, dtype=torch.float64)
    p = torch.softmax(s * scale, -1)
    p.backward(dp)
    pr = R.softmax_fwd(s.detach(), scale)
    assert _err(pr, p.detach()) <= 1e-12 and _err(pr.sum(-1), 1.0) <= 1e-12
    assert _err(R.softmax_bwd(dp, pr, scale), s.grad) <= 1e-12


def test_gelu_grad_reference_matches_autograd():
    torch.manual_seed(2)
    x = torch.cat([torch.tensor([0.0, 1e-3, -1e-3, 1, -1, 6, -6, 12, -12, 40, -40], dtype=torch.float64),
                   torch.randn(500, dtype=torch.float64) * 2]).requires_grad_(True)
    y = F.gelu(x)
    y.sum().backward()
    assert _err(R.gelu(x.detach()), y.detach()) <= 1e-12 and _err(R.gelu_grad(x.detach()), x.grad) <= 1e-12
    assert R.gelu_grad([40.0])[0] == 1.0 and R.gelu_grad([-40.0])[0] == 0.0 and R.gelu_grad([0.0])[0] == 0.5


def _ctc_brute(lp, target, blank):
    """-log of the summed probability of every alignment that collapses to `target` (enumeration; tiny shapes only)."""
    T, V = lp.shape
    tot = 0.0
    for path in itertools.product(range(V), repeat=T):
        col = [k for k, _ in itertools.groupby(path)]
        if [c for c in col if c != blank] == list(target):
            tot += float(np.exp(sum(lp[t, c] for t, c in enumerate(path))))
    return -np.log(tot) if tot > 0 else np.inf


@pytest.mark.parametrize("blank", [0, 2])
def test_ctc_reference(blank):
    torch.manual_seed(3)
    B, T, Tpad, V, S = 4, 5, 8, 3, 4
    a, c = [k for k in range(V) if k != blank]
    logits = torch.randn(B, Tpad, V)
    logits[:, T:] = float("nan")                               # pad frames: never read
    labels = torch.tensor([[a, -100, c, -1], [c, c, -100, -100], [-1, -1, -1, -1], [a, a, a, a]])   # [3]: 7 frames needed
    nll, g = R.ctc_padded(logits, labels, T, blank)
    lp = F.log_softmax(logits[:, :T].double(), -1).numpy()
    want = [_ctc_brute(lp[0], [a, c], blank), _ctc_brute(lp[1], [c, c], blank), _ctc_brute(lp[2], [], blank)]
    assert _err(nll[:3], want) <= 1e-12 and nll[3] == np.inf
    assert np.array_equal(g[:, T:], np.zeros((B, Tpad - T, V))) and np.isnan(g[3, :T]).all() and np.isfinite(g[:3]).all()
    # the gradient of each feasible clip on its own, through autograd of the unpadded call
    for b in range(3):
        x = logits[b:b + 1, :T].double().clone().requires_grad_(True)
        tg = labels[b][labels[b] >= 0]
        F.ctc_loss(F.log_softmax(x, -1).transpose(0, 1), tg, torch.tensor([T]), torch.tensor([len(tg)]), blank=blank,
                   reduction="sum").backward()
        assert _err(g[b, :T], x.grad[0]) <= 1e-12
    # rows of the softmax gradient sum to zero; grad_scale multiplies the result
    assert _err(g[:3, :T].sum(-1), 0.0) <= 1e-12
    for gs in (-1.0, 0.5):
        nll2, g2 = R.ctc_padded(logits, labels, T, blank, gs)
        assert np.array_equal(nll2, nll) and np.array_equal(g2[:3], gs * g[:3]) and np.isnan(g2[3, :T]).all()


def test_planes_helpers():
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((6, 96)) * np.exp(rng.uniform(-20, 20, (6, 96)))).astype(np.float32)
    v[0, :3] = [0.0, -0.0, 1.0]
    hi, none = R.planes_of(v, "hi")
    assert none is None and hi.dtype == np.uint16 and hi.shape == v.shape
    # round to nearest even: |v - hi| <= half a bf16 ulp, ties to the even mantissa
    assert np.all(np.abs(v.astype(np.float64) - bf16_to_f32(hi)) <= np.abs(v.astype(np.float64)) * 2.0 ** -8)
    tie = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=np.float32)
    assert R.planes_of(tie, "hi")[0].tolist() == [0x3F80, 0x3F82]
    h2, lo = R.planes_of(v, "hi+lo")
    assert np.array_equal(h2, hi) and np.array_equal(lo, split_bf16(v)[1])
    # hi + lo reconstructs float32 to 2^-16 relative
    rec = R.planes_value(hi, lo).astype(np.float64)
    assert np.all(np.abs(rec - v) <= np.abs(v.astype(np.float64)) * 2.0 ** -16)
    # the interleaved map: element i of the flat tensor at il_index(i), its lo part 32 further
    il, none = R.planes_of(v, "il")
    assert none is None and il.shape == (6, 192) and np.array_equal(il, interleave_planes(hi, lo))
    idx = R.il_index(np.arange(v.size))
    assert np.array_equal(il.reshape(-1)[idx], hi.reshape(-1)) and np.array_equal(il.reshape(-1)[idx + 32], lo.reshape(-1))
    assert R.il_index([0, 31, 32, 63, 64]).tolist() == [0, 31, 64, 95, 128]
    one = R.planes_of(v.reshape(-1), "il")[0]                   # a flat tensor (paa_mul_gelu_grad_planes): same map
    assert np.array_equal(one, il.reshape(-1))
    with pytest.raises(AssertionError):
        R.planes_of(v[:, :40], "il")


# ---- argument refusals that return before any HIP call (no device needed; the pointers are never dereferenced) --------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from paa_amd import _lib
    return _lib


P = C.c_void_p(4096)          # stands for a device pointer


def test_layernorm_refusals(lib):
    L = lib.lib()
    for cols in (6, 30, 1026):
        assert L.paa_layernorm_fwd(P, P, P, P, P, 2, cols, 1e-5, None) == lib.PAA_ERR_ARG
        assert b"multiple of 4" in L.paa_last_error()
        assert L.paa_layernorm_bwd(P, P, P, P, P, 2, cols, None) == lib.PAA_ERR_ARG
        assert L.paa_layernorm_fwd_planes(P, P, P, P, P, None, None, 0, None, None, 0, None, 2, cols, 1e-5, None) == lib.PAA_ERR_ARG
        assert L.paa_layernorm_bwd_planes(P, P, P, P, None, P, None, None, 0, 2, cols, None) == lib.PAA_ERR_ARG
    # interleaved planes need rows of whole 32-element groups
    for cols in (4, 252, 1028, 48):
        assert L.paa_layernorm_fwd_planes(P, P, P, P, P, P, None, 1, None, None, 0, None, 2, cols, 1e-5, None) == lib.PAA_ERR_ARG
        assert b"multiple of 32" in L.paa_last_error()
        assert L.paa_layernorm_fwd_planes(P, P, P, P, P, None, None, 0, P, None, 1, None, 2, cols, 1e-5, None) == lib.PAA_ERR_ARG
        assert L.paa_layernorm_bwd_planes(P, P, P, P, None, P, P, None, 1, 2, cols, None) == lib.PAA_ERR_ARG
    with pytest.raises(lib.PaaError):
        lib.check(L.paa_layernorm_bwd_planes(P, P, P, P, None, P, P, None, 1, 2, 48, None))


def test_mul_gelu_grad_refusals(lib):
    L = lib.lib()
    for n in (1, 255, 4096 * 256 + 77):
        assert L.paa_mul_gelu_grad_planes(P, P, None, P, None, 1, n, None) == lib.PAA_ERR_ARG
        assert b"multiple of 32" in L.paa_last_error()
    assert L.paa_mul_gelu_grad_planes(P, P, P, None, None, 0, 0, None) == lib.PAA_ERR_ARG


def test_softmax_mats_refusals(lib):
    L = lib.lib()
    assert L.paa_softmax_fwd_mats(P, 2, 8, 7, 4, 4, 1.0, None) == lib.PAA_ERR_ARG       # slot shorter than the matrix
    assert L.paa_softmax_bwd_mats(P, P, 2, 8, 8, 5, 4, 1.0, None) == lib.PAA_ERR_ARG    # ld < cols


def test_ctc_refusals(lib):
    L = lib.lib()

    def both(V, S_max, work):
        a = L.paa_ctc(P, P, 2, 10, V, S_max, 0, 1.0, P, P, work, None)
        b = L.paa_ctc_padded(P, P, 2, 10, 13, V, S_max, 0, 1.0, P, P, None, None, work, None)
        assert a == b
        return a
    assert both(257, 4, P) == lib.PAA_ERR_SIZE and b"vocab" in L.paa_last_error()
    assert both(32, 0, P) == lib.PAA_ERR_SIZE and both(32, 4001, P) == lib.PAA_ERR_SIZE
    assert both(32, 4, C.c_void_p(4096 + 4)) == lib.PAA_ERR_ARG and b"8-byte" in L.paa_last_error()
    assert L.paa_ctc_padded(P, P, 2, 10, 9, 32, 4, 0, 1.0, P, P, None, None, P, None) == lib.PAA_ERR_SIZE     # Tpad < T
    assert L.paa_ctc_padded(P, P, 2, 10, 13, 32, 4, 0, 1.0, P, None, P, P, P, None) == lib.PAA_ERR_ARG        # planes without dlogits
    with pytest.raises(ValueError):
        lib.check(both(257, 4, P))
