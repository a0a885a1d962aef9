"""Float64 statements of the row kernels (csrc/model_kernels.hip k_ln_fwd / k_ln_bwd / k_softmax_fwd / k_softmax_bwd / the CTC
family, csrc/model.hip k_mul_gelu_grad) and of the bf16 plane layouts they write.  Inputs are array-likes or torch tensors of any
float type; every result is a float64 numpy array.  tests/test_rows_ref_host.py checks these against torch float64 autograd."""
import numpy as np
import torch
import torch.nn.functional as F

from paa_amd.model import bf16_bits, bf16_to_f32, interleave_planes, split_bf16

PLANE_MODES = ("hi", "hi+lo", "il")


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64) if not torch.is_tensor(x) else x).double()


def gelu(x):
    """x Phi(x) by erf (torch.nn.functional.gelu(approximate='none'))."""
    x = _t(x)
    return (0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))).numpy()


def gelu_grad(x):
    """Phi(x) + x phi(x)."""
    x = _t(x)
    cdf = 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5))
    pdf = torch.exp(-0.5 * x * x) / (2.0 * np.pi) ** 0.5
    return (cdf + x * pdf).numpy()


def ln_stats(x, eps):
    """(rows, 2): mean and rstd = 1 / sqrt(biased variance + eps) of every row."""
    x = _t(x).numpy()
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return np.stack([mean, 1.0 / np.sqrt(var + eps)], -1)


def ln_fwd(x, g, b, eps):
    """y = (x - mean) rstd g + b, gelu(y), stats (rows, 2)."""
    x, g, b = _t(x).numpy(), _t(g).numpy(), _t(b).numpy()
    st = ln_stats(x, eps)
    y = (x - st[:, :1]) * st[:, 1:] * g + b
    return y, gelu(y), st


def ln_bwd(dy, x, g, stats, add=None):
    """dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) [+ add] with xhat = (x - mean) rstd from the GIVEN stats (rows, 2): the
    gradient of ln_fwd when stats = ln_stats(x, eps), and the same function of slightly different statistics otherwise."""
    dy, x, g, st = _t(dy).numpy(), _t(x).numpy(), _t(g).numpy(), _t(stats).numpy()
    mean, rstd = st[:, :1], st[:, 1:]
    xh = (x - mean) * rstd
    gd = g * dy
    dx = rstd * (gd - gd.mean(-1, keepdims=True) - xh * (gd * xh).mean(-1, keepdims=True))
    return dx if add is None else dx + _t(add).numpy()


def softmax_fwd(s, scale):
    """softmax(scale s) over the last axis."""
    z = _t(s).numpy() * scale
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax_bwd(dp, p, scale):
    """dS = scale P (dP - sum_j dP_j P_j)."""
    dp, p = _t(dp).numpy(), _t(p).numpy()
    return scale * p * (dp - (dp * p).sum(-1, keepdims=True))


def ctc_padded(logits, labels, T, blank, grad_scale=1.0):
    """logits (B, Tpad, V), frames [T, Tpad) never read; labels (B, S_max) integers, the valid ones are the non-negative entries in
    order (masked_select).  Returns nll (B), +inf for a clip without an alignment, and grad_scale * d(sum_b nll_b)/dlogits
    (B, Tpad, V): zero on the pad frames, NaN on the T frames of an infeasible clip (F.ctc_loss(zero_infinity=False) semantics)."""
    lg = torch.as_tensor(np.asarray(logits)) if not torch.is_tensor(logits) else logits
    lab = torch.as_tensor(np.asarray(labels)).long() if not torch.is_tensor(labels) else labels.long()
    B, Tpad, V = lg.shape
    x = lg[:, :T].double().clone().requires_grad_(True)
    lp = F.log_softmax(x, -1).transpose(0, 1)
    mask = lab >= 0
    nll = F.ctc_loss(lp, lab.masked_select(mask), torch.full((B,), T), mask.sum(-1), blank=blank, reduction="none",
                     zero_infinity=False)
    fin = torch.isfinite(nll)
    if bool(fin.any()):
        nll[fin].sum().backward()
    g = torch.zeros(B, Tpad, V, dtype=torch.float64)
    g[:, :T] = x.grad if x.grad is not None else 0.0
    g[~fin, :T] = float("nan")
    nll = nll.detach().clone()
    nll[~fin] = float("inf")
    return nll.numpy(), (g * grad_scale).numpy()


def il_index(i):
    """Position of element i of a tensor whose hi / lo planes are interleaved per 32-element group (csrc/paa_common.h); the lo
    part sits 32 further."""
    i = np.asarray(i, dtype=np.int64)
    return (i >> 5 << 6) + (i & 31)


def planes_of(v, mode):
    """(hi, lo) uint16 planes of a float32 array: hi = bf16(v) round-to-nearest-even; lo = bf16(v - hi) for "hi+lo" (None for
    "hi"); "il": hi is ONE array with both planes interleaved per 32-element group of the last axis (twice as long), lo None."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if mode == "hi":
        return bf16_bits(v), None
    hi, lo = split_bf16(v)
    if mode == "hi+lo":
        return hi, lo
    assert mode == "il" and v.shape[-1] % 32 == 0, (mode, v.shape)
    k = v.shape[-1]
    return interleave_planes(hi.reshape(-1, k), lo.reshape(-1, k)).reshape(v.shape[:-1] + (2 * k,)), None


def planes_value(hi, lo=None):
    """float32 value hi [+ lo] of planar planes."""
    out = bf16_to_f32(np.asarray(hi, dtype=np.uint16))
    return out if lo is None else out + bf16_to_f32(np.asarray(lo, dtype=np.uint16))
