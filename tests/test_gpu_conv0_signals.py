"""-m gpu: conv layer 0 on signals that are not white noise (tests/conv0_ref.py: tones, DC offsets, gated chirp, low-pass noise,
clipping, silence) through a filter bank whose rows cancel on smooth input, against float64.  White noise, the input of every
other test that reaches the conv front end, is the one signal on which the Gram-matrix evaluation of the GroupNorm statistics
(k_conv0_gram / k_conv0_gn_stats: var_c = w_c^T G w_c / T - mean_c^2) is perfectly conditioned.

Every signal is one clip of one batch; the perturbation is a zero row.  L = 8000 is one Gram chunk, L = 10250 gives
T0 = 2049: a full chunk and a one-frame tail."""
import numpy as np
import pytest
import torch

import conv0_ref as R
from oracle import pgd as opgd, trace, wav2vec2 as OW
from oracle.gen_cases import cli_to_args
from paa_amd import arch as A
from paa_amd.model import PaaModel
from test_gpu_model import ACT_TOL, GRAD_TOL
from test_lengths import texts_for

pytestmark = pytest.mark.gpu

LENGTHS = (8000, 10250)
DTYPES = ("fp32", "bf16")
NAMES = ("white", "tone120", "tone_dc", "chirp_gated", "lowpass", "dc_only", "zeros", "clipped")
B = len(NAMES)
EPS = 1e-5
FE0 = "wav2vec2.feature_extractor.conv_layers.0"

_cache = {}


def _arch(kind):
    return A.tiny("group", False, conv_dim=(32,) * 7) if kind == "group" else A.tiny("layer", True, conv_dim=(32,) * 7)


def _weights(kind):
    """rule_weights with conv layer 0's weight replaced by the filter bank (gamma, beta and the conv bias as the rule made them)."""
    key = ("sd", kind)
    if key not in _cache:
        sdn = A.rule_weights(_arch(kind))
        sdn[f"{FE0}.conv.weight"] = R.filter_bank(32).reshape(32, 1, 10).copy()
        _cache[key] = sdn
    return _cache[key]


def _clips(L):
    key = ("clips", L)
    if key not in _cache:
        s = R.signals(L)
        assert tuple(s) == NAMES
        _cache[key] = np.stack([s[n] for n in NAMES])
    return _cache[key]


def _labels(a, L):
    return opgd.make_labels((texts_for(a, L, 4) * 2)[:B], cli_to_args("snr", []), B)


def _run(kind, L, dtype):
    """One forward/backward of the whole batch, shared by the tests: gn_stats, conv0.pre / conv0.act in the padded layout, the
    waveform gradient."""
    key = (kind, L, dtype)
    if key not in _cache:
        a = _arch(kind)
        m = PaaModel(a, _weights(kind), B, L, dtype)
        clean = torch.from_numpy(_clips(L)).cuda()
        r = m.fwd_bwd(clean, torch.zeros(1, L, device="cuda"), _labels(a, L), +1)
        torch.cuda.synchronize()
        P0, T0 = m.layout(0), a.feat_lengths(L)[0]
        assert T0 == R.n_frames(L) and P0 >= T0
        out = dict(P0=P0, T0=T0, loss=float(r["loss"]), grad=r["grad"].cpu().numpy().copy(),
                   pre=m.debug_read("conv0.pre", B).reshape(B, P0, 32).copy(),
                   act=m.debug_read("conv0.act", B).reshape(B, P0, 32).copy())
        if kind == "group":
            out["gn_stats"] = m.debug_read("gn_stats", B).reshape(B, 32, 2).copy()
        _cache[key] = out
    return _cache[key]


def _ref64(kind, L):
    """float64 (y, gelu(y), gelu'(y) | None) per clip, computed once per length."""
    key = ("ref", kind, L)
    if key not in _cache:
        sdn, W = _weights(kind), R.filter_bank(32)
        g, b = sdn[f"{FE0}.layer_norm.weight"], sdn[f"{FE0}.layer_norm.bias"]
        if kind == "group":
            _cache[key] = [R.conv0_64(x, W, g, b, EPS) for x in _clips(L)]
        else:
            _cache[key] = [R.conv0_ln64(x, W, sdn[f"{FE0}.conv.bias"], g, b, EPS) + (None,) for x in _clips(L)]
    return _cache[key]


def _chan_err(got, ref):
    """Per channel of one clip: max_t |got - ref| / max_t |ref| — a quiet channel is measured against itself."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref).max(axis=0)
    return d / np.maximum(np.abs(ref).max(axis=0), 1e-30)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LENGTHS)
def test_gn_stats_vs_float64(L, dtype):
    """Per clip, worst channel: the kernel's rstd (relative) and mean (as it lands on the normalised output) errors e_k against
    float64, bounded by 4 * e_32 + 5e-7 with e_32 the same errors of a plain float32 evaluation (conv, mean, variance of the
    outputs).  4: two f32 evaluations that differ in summation order; 5e-7: a few f32 ulps for the final casts.

    Measured on an MI355X, rstd e_k, worst channel (L = 8000 / 10250; the same bits in both modes), e_32 between 5e-8 and 9e-7:
      Gram products formed in f32 (before): white 5.3e-8, tone120 6.25e-4 / 4.19e-4, tone_dc 2.83e-4 / 3.04e-4, chirp_gated
        3.99e-5 / 1.16e-5, lowpass 6.4e-7 / 4.8e-7, dc_only 4.87e-3 / 1.00e-2, zeros 5.4e-8, clipped 5.18e-4 / 4.74e-4: the test
        failed on tone120, tone_dc, chirp_gated, dc_only and clipped (and on tone_dc's mean: 2.1e-6 / 4.2e-6 against e_32 5e-7)
      products and sums in f64 (now): <= 6.0e-8 on every clip, the rounding of the stored f32; mean <= 1.3e-7, and 8.8e-6 on
        dc_only (half an ulp of a mean of 0.3 over sqrt(eps); e_32 3.2e-5 there)."""
    got = _run("group", L, dtype)["gn_stats"]
    W = R.filter_bank(32)
    bad = []
    for b, name in enumerate(NAMES):
        x = _clips(L)[b]
        ref = R.stats64(x, W, EPS)
        km, kr = R.stats_err((got[b, :, 0], got[b, :, 1]), ref, EPS)
        fm, fr = R.stats_err(R.stats32(x, W, EPS), ref, EPS)
        print(f"L={L} {dtype} {name:12s} rstd e_k {kr.max():.2e} (ch {kr.argmax():2d}) e_32 {fr.max():.2e} | "
              f"mean e_k {km.max():.2e} (ch {km.argmax():2d}) e_32 {fm.max():.2e}")
        if not kr.max() <= 4 * fr.max() + 5e-7:
            bad.append((name, "rstd", float(kr.max()), float(fr.max())))
        if not km.max() <= 4 * fm.max() + 5e-7:
            bad.append((name, "mean", float(km.max()), float(fm.max())))
    assert np.isfinite(got).all()
    assert not bad, bad


@pytest.mark.parametrize("L", LENGTHS)
def test_stats_are_per_clip_and_mode_independent(L):
    """The Gram sums are per clip, in a fixed order, from the f32 samples alone: a clip's (mean, rstd) row is the same bits
    inside the batch and alone (B = 1), and the same bits in the fp32-parity and the bf16 model."""
    a = _arch("group")
    rows = {d: _run("group", L, d)["gn_stats"] for d in DTYPES}
    assert np.array_equal(rows["fp32"], rows["bf16"])
    for dtype in DTYPES:
        m = PaaModel(a, _weights("group"), 1, L, dtype)
        for b, name in enumerate(NAMES):
            clean = torch.from_numpy(_clips(L)[b:b + 1].copy()).cuda()
            m.forward(clean, None, None, want_logits=False)
            torch.cuda.synchronize()
            alone = m.debug_read("gn_stats", 1).reshape(32, 2)
            assert np.array_equal(alone, rows[dtype][b]), (dtype, name)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LENGTHS)
def test_conv0_activations_vs_float64(L, dtype, name):
    """conv0.act against gelu(y) and conv0.pre against gelu'(y) (the "group" model keeps the gate in both modes), y the float64
    GroupNorm of the float64 conv: relative error per channel of the clip, worst channel, at test_gpu_model's ACT_TOL; the padded
    rows [T0, P0) exactly zero.

    Measured on an MI355X, conv0.act, fp32, worst channel (L = 8000 / 10250); bf16 is 3.0e-3 .. 4.1e-3 throughout (1.1e-2 dc_only):
      before (f32 Gram products): tone120 7.8e-4 / 5.3e-4, tone_dc 2.8e-4 / 3.2e-4, clipped 5.2e-4 / 4.7e-4 (over 3e-4), dc_only 1.2e-2
      exact statistics, conv of the raw samples: tone120 5.4e-5, tone_dc 8.8e-5, clipped 6.4e-6 — and dc_only still 1.2e-2
      now (samples centred on the clip mean): white 5.7e-6 / 6.7e-6, tone120 1.1e-4 / 7.2e-5, tone_dc 3.4e-5 / 3.1e-5, chirp_gated
        7e-6, lowpass 7e-6, dc_only 5.4e-6, zeros 5.4e-6, clipped 6.4e-6 / 7.4e-6

    dc_only is what the centring in k_conv0_gn is for.  On a constant clip every frame's conv output v is the same number, the
    float64 reference is y = beta exactly, and gelu(beta_c) is as small as 4e-5.  A chain of ten f32 fmas over the raw samples
    is off the exact v by about 1e-8; the mean it is compared with is exact, so the residue survived and was multiplied by
    rstd = 1 / sqrt(eps) = 316: an absolute 5e-6, 1.2e-2 of a reference that small (a float32 torch evaluation: 4.4e-4).  With the
    clip mean taken off the samples first, v - mean is formed from x - m and its rounding vanishes with the signal's variation."""
    r = _run("group", L, dtype)
    b = NAMES.index(name)
    y, act, gate = _ref64("group", L)[b]
    T0, P0 = r["T0"], r["P0"]
    e_act, e_pre = _chan_err(r["act"][b, :T0], act), _chan_err(r["pre"][b, :T0], gate)
    print(f"L={L} {dtype} {name:12s} conv0.act {e_act.max():.2e} (ch {e_act.argmax():2d}) conv0.pre {e_pre.max():.2e} (ch {e_pre.argmax():2d})")
    assert np.all(r["act"][b, T0:P0] == 0) and np.all(r["pre"][b, T0:P0] == 0)
    assert np.isfinite(r["act"][b]).all() and np.isfinite(r["pre"][b]).all()
    assert e_act.max() < ACT_TOL[dtype] and e_pre.max() < ACT_TOL[dtype], (float(e_act.max()), float(e_pre.max()))


@pytest.mark.parametrize("L", LENGTHS)
def test_waveform_gradient_on_signals(L):
    """fp32-parity mode: d loss / d perturbation (a zero row: the sum over the clips) against the oracle run in float64; e_32 is
    the float32 oracle's own error against it.  The kernel's error stays within max(GRAD_TOL, 4 * e_32).
    Measured (L = 8000 / 10250): e_k 2.9e-5 / 3.2e-5, e_32 4.3e-5 / 3.7e-5; with the f32 Gram products e_k was 5.4e-4 / 1.18e-3
    (inside GRAD_TOL: the sum over eight clips hides the tonal ones), with exact statistics and uncentred samples 1.0e-4."""
    a = _arch("group")
    labels = _labels(a, L)
    grads = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.to(dt) for k, v in OW.to_torch(_weights("group")).items()}
        p = torch.zeros(1, L, dtype=dt, requires_grad=True)
        loss, _ = trace.forward_trace(sd, a, (torch.from_numpy(_clips(L)).to(dt) + p).clamp(-1, 1), labels, direction=1.0)
        grads[dt] = (p.grad.double().numpy().copy(), float(loss))
    g64, l64 = grads[torch.float64]
    r = _run("group", L, "fp32")
    scale = np.abs(g64).max()
    e_k = float(np.abs(r["grad"].astype(np.float64) - g64).max() / scale)
    e_32 = float(np.abs(grads[torch.float32][0] - g64).max() / scale)
    print(f"L={L} fp32 grad: e_k {e_k:.2e} e_32 {e_32:.2e}; loss {r['loss']:.6f} (f64 oracle {l64:.6f})")
    assert np.isfinite(l64) and scale > 0 and np.isfinite(r["grad"]).all()
    assert abs(r["loss"] - l64) <= ACT_TOL["fp32"] * abs(l64)
    assert e_k <= max(GRAD_TOL["fp32"], 4 * e_32)
    tail = (r["T0"] - 1) * 5 + 10
    assert np.all(r["grad"][:, tail:] == 0)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LENGTHS)
def test_layernorm_conv0_control(L, dtype, name):
    """Control: the same batch and filter bank through the "layer" extractor (k_conv0_rows, a two-pass per-frame LayerNorm over
    the channels): conv0.pre (the normalised pre-activation) and conv0.act against float64, same measure and tolerance.
    Measured: fp32 conv0.act <= 7.3e-6, conv0.pre <= 6.6e-6 on every clip; bf16 conv0.act <= 3.8e-3."""
    r = _run("layer", L, dtype)
    b = NAMES.index(name)
    y, act, _ = _ref64("layer", L)[b]
    T0, P0 = r["T0"], r["P0"]
    e_act, e_pre = _chan_err(r["act"][b, :T0], act), _chan_err(r["pre"][b, :T0], y)
    print(f"L={L} {dtype} {name:12s} layer conv0.act {e_act.max():.2e} (ch {e_act.argmax():2d}) conv0.pre {e_pre.max():.2e} (ch {e_pre.argmax():2d})")
    assert np.all(r["act"][b, T0:P0] == 0) and np.all(r["pre"][b, T0:P0] == 0)
    assert e_act.max() < ACT_TOL[dtype] and e_pre.max() < ACT_TOL[dtype], (float(e_act.max()), float(e_pre.max()))
