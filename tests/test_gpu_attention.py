"""-m gpu: the fused attention kernels (csrc/attention.hip) and the materialised softmax (model_kernels.hip) against
float64, at the model's shapes and at the edges where such kernels go wrong.

Errors are measured per (clip, head, tensor): max|err| / max|ref| over the head's valid rows, so an error confined to one
head or to a head of small magnitude cannot hide behind the largest head of the call.  Saturated dQ / dK blocks are held
to the same bound relative to their natural scale (see SAT below).  Every output buffer starts out filled with a NaN
sentinel: positions the kernels must not write have to keep it, positions they must write must not."""
import numpy as np
import pytest
import torch

import attn_ref as R
from paa_amd import _lib
from paa_amd.model import bf16_to_f32

pytestmark = pytest.mark.gpu

# (B, nh, T, P - T, Tp - ceil32(T)): T = 1, the 32 / 64 / 128 tile edges, a tail group of heads (nh = 12 -> 8 + 4), full
# groups of 8, padded layouts, 10 s (T = 499) and 30 s (T = 1499) clips.  Heads take the patterns of attn_ref in turn.
SHAPES = [(1, 1, 1, 1, 0), (2, 1, 2, 3, 0), (1, 12, 63, 1, 32), (1, 8, 64, 5, 0), (2, 12, 65, 1, 0), (3, 16, 129, 7, 0),
          (2, 12, 499, 3, 0), (1, 16, 1499, 1, 0)]
CEIL = {"bf16": {"o": 1e-2, "dq": 2e-2, "dk": 2e-2, "dv": 2e-2},
        "split": {"o": 5e-5, "dq": 1e-4, "dk": 1e-4, "dv": 1e-4}}
# Bounds, set at about 3.5x the worst block measured on an MI355X and never above CEIL.  Worst measured, max|err| / max|ref|
# per block: bf16 O 5.6e-3, dQ 5.8e-3, dK 6.1e-3, dV 5.4e-3 (output rounding alone is up to 2^-9 = 2e-3);
# split O 1.9e-5, dQ 1.5e-5, dK 1.8e-5, dV 3.9e-5 (the last two in negshift heads, O and dQ 1.2e-5, 1.5e-5 in random ones).
TIGHT = {"bf16": CEIL["bf16"], "split": {"o": 5e-5, "dq": 5e-5, "dk": 6e-5, "dv": 1e-4}}
# Saturated dQ / dK blocks (kappa > KAPPA_SAT: peaked and dominant rows, where dS ~ P (1 - P), and heads whose keys or
# queries share a large component that the gradient sums to zero) lose digits to any rounding of the terms they are
# summed from: the split products' dropped lo*lo term and hi + lo O (delta), the bf16 mode's P, dS and O.  A float64
# emulation of that arithmetic (attn_ref.attn_emulated) reproduces the measured errors head by head.  Against the exact
# reference they are held at measured bounds (worst: bf16 dQ 1.0, dK 2.2; split dQ 2.2e-3, dK 7.0e-3), and against their
# natural scale (attn_ref.attn_ref: nat) at TIGHT, like every well-conditioned block.
KAPPA_SAT = 12.0
SAT = {"bf16": {"dq": 4.0, "dk": 8.0}, "split": {"dq": 8e-3, "dk": 2.5e-2}}
# T = 1: the exact dQ and dK are 0; the kernels' are bounded by the cancellation scale of dP - delta (worst: bf16 0, split 3e-7)
T1_BOUND = {"bf16": 1e-6, "split": 1e-6}
TENSORS = ("o", "dq", "dk", "dv")


def _dims(shape):
    B, nh, T, dp, dtp = shape
    return B, nh, T, T + dp, -(-T // 32) * 32 + dtp


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _sentinel16(*shape):
    return torch.full(shape, R.NAN16, dtype=torch.int16, device="cuda")


def _sentinel32(*shape):
    return torch.full(shape, R.NAN32, dtype=torch.int32, device="cuda").view(torch.float32)


def run_attention(inp, B, nh, T, P, Tp):
    """Forward then backward on the planes of `inp` (attn_ref.build_inputs); every output starts as the sentinel.
    Returns host arrays: ctx / dqkv planes as uint16 bits (lo planes None in bf16 mode), lse / delta as float32."""
    split = inp["qkv_lo"] is not None
    H = nh * R.HD
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    qh, dh = _dev16(inp["qkv_hi"]), _dev16(inp["do_hi"])
    ch, gh = _sentinel16(B * P, H), _sentinel16(B * P, 3 * H)
    lse, delta = _sentinel32(B * nh, Tp), _sentinel32(B * nh, Tp)
    if split:
        ql, dl = _dev16(inp["qkv_lo"]), _dev16(inp["do_lo"])
        cl, gl = _sentinel16(B * P, H), _sentinel16(B * P, 3 * H)
        _lib.check(L.paa_attn_fwd_split(p(qh), p(ql), p(ch), p(cl), p(lse), B, T, P, Tp, H, nh, st))
        _lib.check(L.paa_attn_bwd_split(p(qh), p(ql), p(ch), p(cl), p(lse), p(dh), p(dl), p(delta), p(gh), p(gl),
                                        B, T, P, Tp, H, nh, st))
    else:
        cl = gl = None
        _lib.check(L.paa_attn_fwd(p(qh), p(ch), p(lse), B, T, P, Tp, H, nh, st))
        _lib.check(L.paa_attn_bwd(p(qh), p(ch), p(lse), p(dh), p(delta), p(gh), B, T, P, Tp, H, nh, st))
    torch.cuda.synchronize()
    host16 = lambda t: None if t is None else t.cpu().numpy().view(np.uint16)
    return {"ctx_hi": host16(ch), "ctx_lo": host16(cl), "dqkv_hi": host16(gh), "dqkv_lo": host16(gl),
            "lse": lse.cpu().numpy(), "delta": delta.cpu().numpy()}


def _value(hi, lo):
    v = bf16_to_f32(hi).astype(np.float64)
    return v if lo is None else v + bf16_to_f32(lo)


def _err(got, ref):
    """max|got - ref| / max|ref|; a reference that is exactly zero must be matched exactly."""
    num, den = np.abs(got - ref).max(), np.abs(ref).max()
    return num / den if den > 0 else (0.0 if num == 0 else np.inf)


def _check_untouched(out, B, P, T):
    """Rows [T, P) of every clip in ctx / dqkv and entries [T, Tp) of lse / delta still hold the sentinel."""
    for name in ("ctx_hi", "ctx_lo", "dqkv_hi", "dqkv_lo"):
        if out[name] is not None:
            assert (out[name].reshape(B, P, -1)[:, T:] == R.NAN16).all(), f"{name}: write into a pad row"
    for name in ("lse", "delta"):
        assert (out[name].view(np.uint32)[:, T:] == R.NAN32).all(), f"{name}: write past T"


def _head_outputs(out, b, h, B, nh, T, P):
    """The kernel's o, dq, dk, dv of head (b, h), rows < T, float64."""
    H = nh * R.HD
    ctx = _value(out["ctx_hi"], out["ctx_lo"]).reshape(B, P, H)[b, :T]
    g = _value(out["dqkv_hi"], out["dqkv_lo"]).reshape(B, P, 3 * H)[b, :T]
    cs = lambda i: slice(i * H + h * R.HD, i * H + (h + 1) * R.HD)
    return {"o": ctx[:, cs(0)], "dq": g[:, cs(0)], "dk": g[:, cs(1)], "dv": g[:, cs(2)]}


@pytest.mark.parametrize("mode", ["bf16", "split"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}nh{}T{}P+{}Tp+{}".format(*s))
def test_attention_parity_sweep(mode, shape):
    B, nh, T, P, Tp = _dims(shape)
    split = mode == "split"
    inp = R.build_inputs(B, nh, T, P, Tp, split, seed=1000 * T + B * nh)
    out = run_attention(inp, B, nh, T, P, Tp)
    _check_untouched(out, B, P, T)
    for name in ("ctx", "dqkv"):
        v = _value(out[name + "_hi"], out[name + "_lo"]).reshape(B, P, -1)[:, :T]
        assert np.isfinite(v).all(), f"{name}: NaN / Inf (or an unwritten position) in rows < T"
    for name in ("lse", "delta"):
        assert np.isfinite(out[name][:, :T]).all(), f"{name}: NaN / Inf (or an unwritten entry) below T"
    lse, delta = out["lse"].reshape(B, nh, -1), out["delta"].reshape(B, nh, -1)
    worst, bad = {}, []

    def record(key, e, bound, what):
        worst[key] = max(worst.get(key, 0.0), e)
        if not e <= bound:
            bad.append(f"{what} {e:.2e} > {bound:.0e}")

    for b in range(B):
        for h in range(nh):
            pat = inp["patterns"][b * nh + h]
            tag = f"({b},{h}) {pat}"
            q, k, v = R.head_slices(inp["qkv"][b], nh, h)
            do = inp["do"][b][:, h * R.HD:(h + 1) * R.HD]
            ref = R.attn_ref(q, k, v, do)
            got = _head_outputs(out, b, h, B, nh, T, P)
            record((pat, "lse"), float((np.abs(lse[b, h, :T] - ref["lse"]) / np.maximum(1.0, np.abs(ref["lse"]))).max()),
                   1e-4, f"{tag} lse")
            # delta is rowsum(dO * O) over the kernel's own stored O; per row, relative to sum |dO * O|
            prod = do * got["o"]
            record((pat, "delta"), float((np.abs(delta[b, h, :T] - prod.sum(1)) / np.abs(prod).sum(1)).max()), 1e-5,
                   f"{tag} delta")
            for t in TENSORS:
                if T == 1 and t in ("dq", "dk"):    # exact reference 0: bounded by the cancellation scale of dP - delta
                    nat = R.SCALE * np.abs(do * v).sum() * np.abs(k if t == "dq" else q).max()
                    record((pat, t), float(np.abs(got[t]).max() / nat), T1_BOUND[mode], f"{tag} {t} (T = 1)")
                    continue
                if t in ref["kappa"] and ref["kappa"][t] > KAPPA_SAT:
                    record((pat, t + "/sat"), float(_err(got[t], ref[t])), SAT[mode][t], f"{tag} {t} (saturated)")
                    record((pat, t + "/nat"), float(np.abs(got[t] - ref[t]).max() / ref["nat"][t].max()), TIGHT[mode][t],
                           f"{tag} {t} (saturated) against its natural scale")
                else:
                    record((pat, t), float(_err(got[t], ref[t])), TIGHT[mode][t], f"{tag} {t}")
            if pat == "flat" and not (got["dk"] == 0).all():
                bad.append(f"{tag}: dK not exactly 0")
    for (pat, t), e in sorted(worst.items()):
        print(f"ATTN {mode} B={B} nh={nh} T={T} {pat:13s} {t:10s} {e:.2e}")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------ bit-exact invariants
# 3 clips x 12 heads = 36 (clip, head) pairs: four groups of 8 in attn_block's grouped order and a tail of 4; T = 200 gives
# two 128-position blocks per head.  A clip alone (12 heads: one group and a tail) and a head alone (1 head: tail only)
# take other workgroup orders, but each (clip, head, block) does the same arithmetic, so the bits must agree.
INV = (3, 12, 200, 5, 32)
_inv_cache = {}


def _inv_batch(mode):
    if mode not in _inv_cache:
        B, nh, T, P, Tp = _dims(INV)
        inp = R.build_inputs(B, nh, T, P, Tp, mode == "split", seed=77)
        _inv_cache[mode] = (inp, run_attention(inp, B, nh, T, P, Tp))
    return _inv_cache[mode]


def _same(a, b):
    return a is None and b is None or np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                     b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("mode", ["bf16", "split"])
def test_attention_clip_alone_is_bit_exact(mode):
    B, nh, T, P, Tp = _dims(INV)
    inp, out = _inv_batch(mode)
    for b in (0, B - 1):
        sub = {k: (None if v is None else v.reshape(B, P, -1)[b]) for k, v in inp.items() if k.endswith(("_hi", "_lo"))}
        one = run_attention(sub, 1, nh, T, P, Tp)
        for name in ("ctx_hi", "ctx_lo", "dqkv_hi", "dqkv_lo"):
            assert _same(None if out[name] is None else out[name].reshape(B, P, -1)[b], one[name]), (b, name)
        for name in ("lse", "delta"):
            assert _same(out[name].reshape(B, nh, Tp)[b], one[name]), (b, name)


@pytest.mark.parametrize("mode", ["bf16", "split"])
def test_attention_head_alone_is_bit_exact(mode):
    B, nh, T, P, Tp = _dims(INV)
    H = nh * R.HD
    inp, out = _inv_batch(mode)
    cs = lambda i, h: slice(i * H + h * R.HD, i * H + (h + 1) * R.HD)
    # (clip, head) -> flat head 0 (first group), 16 (third group), 33 and 35 (the tail group; 35 is the last head)
    for b, h in ((0, 0), (1, 4), (2, 9), (2, 11)):
        sub = {}
        for pl in ("_hi", "_lo"):
            x, d = inp["qkv" + pl], inp["do" + pl]
            if x is None:
                sub["qkv" + pl] = sub["do" + pl] = None
                continue
            x, d = x.reshape(B, P, 3 * H)[b], d.reshape(B, P, H)[b]
            sub["qkv" + pl] = np.concatenate([x[:, cs(i, h)] for i in range(3)], axis=1)
            sub["do" + pl] = d[:, cs(0, h)]
        one = run_attention(sub, 1, 1, T, P, Tp)
        for pl in ("_hi", "_lo"):
            if out["ctx" + pl] is None:
                continue
            assert _same(np.ascontiguousarray(out["ctx" + pl].reshape(B, P, H)[b][:, cs(0, h)]), one["ctx" + pl]), (b, h)
            g = out["dqkv" + pl].reshape(B, P, 3 * H)[b]
            assert _same(np.ascontiguousarray(np.concatenate([g[:, cs(i, h)] for i in range(3)], axis=1)), one["dqkv" + pl]), (b, h)
        for name in ("lse", "delta"):
            assert _same(np.ascontiguousarray(out[name].reshape(B, nh, Tp)[b, h:h + 1]), one[name]), (b, h, name)


@pytest.mark.parametrize("mode", ["bf16", "split"])
def test_attention_is_deterministic(mode):
    B, nh, T, P, Tp = _dims(INV)
    inp, out = _inv_batch(mode)
    again = run_attention(inp, B, nh, T, P, Tp)
    for name, a in out.items():
        assert _same(a, again[name]), name


# ------------------------------------------------------------------------------------------ exact edges
def test_attention_single_key_bf16():
    """T = 1: P = 1 exactly, so O is V bit for bit, lse is c s_00, dV is dO bit for bit and dQ = dK = 0 up to the rounding
    of dP - delta."""
    B, nh, T, P, Tp = 2, 12, 1, 3, 32
    H = nh * R.HD
    inp = R.build_inputs(B, nh, T, P, Tp, False, seed=11, patterns=["random"] * (B * nh))
    out = run_attention(inp, B, nh, T, P, Tp)
    _check_untouched(out, B, P, T)
    qkv, ctx, g = inp["qkv_hi"].reshape(B, P, 3 * H), out["ctx_hi"].reshape(B, P, H), out["dqkv_hi"].reshape(B, P, 3 * H)
    assert np.array_equal(ctx[:, 0], qkv[:, 0, 2 * H:])
    assert np.array_equal(g[:, 0, 2 * H:], inp["do_hi"].reshape(B, P, H)[:, 0])
    lse = out["lse"].reshape(B, nh, Tp)[:, :, 0]
    for b in range(B):
        for h in range(nh):
            q, k, v = R.head_slices(inp["qkv"][b], nh, h)
            do = inp["do"][b][:, h * R.HD:(h + 1) * R.HD]
            s00 = float(R.scores2(q, k)[0, 0])
            assert abs(lse[b, h] - s00) <= 1e-4 * max(1.0, abs(s00))
            got = _head_outputs(out, b, h, B, nh, T, P)
            nat = R.SCALE * np.abs(do * v).sum()
            assert np.abs(got["dq"]).max() <= 1e-5 * nat * np.abs(k).max()
            assert np.abs(got["dk"]).max() <= 1e-5 * nat * np.abs(q).max()


# ------------------------------------------------------------------------------------------ materialised softmax
# paa_softmax_fwd / _bwd: the attention path of head dims other than 64 (the tiny test models: 4 heads of 16, scale 1/4).
# Rows cycle through random, peaked (one entry leads by ~6 nats + log cols), constant and strongly negative scores.
@pytest.mark.parametrize("cols", [1, 31, 64, 65, 499, 1499])
def test_softmax_rows_and_pad_columns(cols):
    rows, ld, scale = 37, cols + 33, 0.25
    rng = np.random.default_rng(cols)
    s = rng.standard_normal((rows + 3, ld)).astype(np.float32) * 3
    kind = np.arange(rows) % 4
    for r in range(rows):
        if kind[r] == 1:
            s[r, rng.integers(0, cols)] += (np.log(cols) + 6.0) / scale
        elif kind[r] == 2:
            s[r] = 2.5
        elif kind[r] == 3:
            s[r] -= 3000.0
    dp = rng.standard_normal((rows + 3, ld)).astype(np.float32)
    nan = np.float32(np.uint32(R.NAN32).view(np.float32))
    s[:, cols:] = nan
    dp[:, cols:] = nan
    s[rows:] = nan                                           # rows past `rows` must stay untouched
    dp[rows:] = nan
    x = s[:rows, :cols].astype(np.float64) * scale
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    d = dp[:rows, :cols].astype(np.float64)
    ds = scale * p * (d - (d * p).sum(1, keepdims=True))
    sd, dpd = torch.from_numpy(s).cuda(), torch.from_numpy(dp).cuda()
    L = _lib.lib()
    _lib.check(L.paa_softmax_fwd(_lib.ptr(sd), rows, cols, ld, scale, _lib.stream_ptr()))
    _lib.check(L.paa_softmax_bwd(_lib.ptr(dpd), _lib.ptr(sd), rows, cols, ld, scale, _lib.stream_ptr()))
    torch.cuda.synchronize()
    pg, dg = sd.cpu().numpy(), dpd.cpu().numpy()
    assert (pg[:rows, cols:] == 0).all() and (dg[:rows, cols:] == 0).all()
    assert (pg[rows:].view(np.uint32) == R.NAN32).all() and (dg[rows:].view(np.uint32) == R.NAN32).all()
    # the backward's own contract: scale * P * (dP - sum dP P) for the P it is given (the forward's output)
    pk = pg[:rows, :cols].astype(np.float64)
    dot = (d * pk).sum(1, keepdims=True)
    dsk = scale * pk * (d - dot)
    nat = scale * pk * (np.abs(d) + np.abs(dot))          # what the rounding of dP - sum dP P scales with
    e1 = np.array([_err(pg[r, :cols], p[r]) for r in range(rows)])
    e2 = np.array([_err(dg[r, :cols], ds[r]) for r in range(rows)])
    e3 = np.array([np.abs(dg[r, :cols] - dsk[r]).max() / nat[r].max() for r in range(rows)])
    for kd, name in enumerate(("random", "peaked", "constant", "negative")):
        print(f"\nSOFTMAX cols={cols} {name:9s} fwd {e1[kind == kd].max():.2e} bwd {e2[kind == kd].max():.2e} "
              f"natural scale {e3[kind == kd].max():.2e}")
    # worst measured: fwd 4.1e-7; bwd 2.4e-7 (peaked rows 1.8e-4: f32 dP - sum dP P cancels), 1.4e-7 of the natural scale
    assert e1.max() < 1.5e-6 and e2[kind != 1].max() < 1e-6 and e2[kind == 1].max() < 7e-4 and e3.max() < 5e-7
