"""-m gpu: the label-free feature-distance loss — paa_feature_cos against tests/feature_ref.py, the hidden state's
way out of the model (paa_model_features, PaaModel.features), the loss inside the training calls (paa_model_set_feature_loss), the
two device steps and the two runners under --loss_type feature.  Tiny rule-weight architectures: B = 3 clips of L = 8000 samples
(24 frames).

  paa_feature_cos   per row at most 4 x the error torch float32 makes on the CPU against the same float64 reference, floor 4 ulp
                    of the row's largest output: the rule of tests/test_gpu_rows.py (row_bound), not re-chosen
  features          ACT_TOL of tests/test_gpu_model.py, what it applies to the logits of the same architecture and dtype
  stats[0], nll     2^-22 relative, as tests/test_gpu_margin_step.py: float32 roundings of d (2^-24 each), a float64 sum, one more
  grad wrt p        against the oracle's autograd with the reference's cotangent injected at the hidden state, GRAD_TOL of
                    tests/test_gpu_model.py
  rows / solo       1e-5, the bound tests/test_gpu_clip_attack.py::test_model_rows sets for a row against the batch-1 call
  steps             eager steps equal the hand-sequenced calls, and captured steps the eager ones, bit for bit"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import feature_ref as FR
from gpu_util import rel_err
from oracle import pgd as opgd, wav2vec2 as OW
from oracle.gen_cases import cli_to_args
from paa_amd import _lib, arch as A, attack_clips, run_attack, runtime, synth
from paa_amd.core import features as core_features
from paa_amd.model import PaaModel
from paa_amd.training_utils import parser
from paa_amd.training_utils.clip_attack import ClipStepper
from paa_amd.training_utils.pgd import PgdStepper
from test_gpu_model import ACT_TOL, GRAD_TOL
from test_gpu_rows import Guarded, over, row_bound, row_err, same_bits

pytestmark = pytest.mark.gpu

B, L, T = 3, 8000, 24
HD64 = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256)      # head dim 64: the fused attention path lengths need
LOSS_RTOL = 2.0 ** -22
ARG, SIZE = _lib.PAA_ERR_ARG, _lib.PAA_ERR_SIZE


def _arch(variant, hd64=False):
    kw = HD64 if hd64 else {}
    return A.tiny("group", False, **kw) if variant == "group" else A.tiny("layer", True, **kw)


# ================================================================================ paa_feature_cos ===
H_ROWS = 32
DEG_H, DEG_R, NEAR = (0, 3), (1, 5), (2, 0)          # an all-zero h row, an all-zero ref row, a row with h almost equal to ref


def _cos_inputs(H, seed=7):
    g = torch.Generator().manual_seed(seed + H)
    h = torch.randn(B, H_ROWS, H, generator=g)
    r = torch.randn(B, T, H, generator=g) * 2.0 + 0.1
    h[DEG_H] = 0.0
    r[DEG_R] = 0.0
    h[NEAR] = r[NEAR] + 1e-3 * torch.randn(H, generator=g)
    h[:, T:] = float("nan")                           # the pad rows of h are not read
    return h, r


def _call(h, r, frames, H, gs, dist=True, dh=True):
    """One call on guarded outputs -> dict(status, loss, dist, dh as numpy | None)."""
    Lb = _lib.lib()
    hd, rd = h.cuda(), r.cuda()
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device="cuda")
    loss, work = Guarded((B,)), Guarded((int(Lb.paa_feature_cos_work_floats(B, T)),))
    gd = Guarded((B, T)) if dist else None
    gh = Guarded((B, H_ROWS, H)) if dh else None
    st = Lb.paa_feature_cos(_lib.ptr(hd), H_ROWS, _lib.ptr(rd), T, _lib.ptr(fr), B, T, H, float(gs), loss.ptr,
                            gd.ptr if gd else None, gh.ptr if gh else None, work.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    for x in (loss, work, gd, gh):
        if x is not None:
            x.check()
    return dict(status=st, loss=loss.numpy(), dist=gd.numpy() if gd else None, dh=gh.numpy() if gh else None)


@pytest.mark.parametrize("frames", [None, [24, 7, 1]], ids=["full", "frames"])
@pytest.mark.parametrize("H", [64, 72, 768, 1024])
def test_feature_cos_vs_reference(H, frames):
    gs = -1.5
    h, r = _cos_inputs(H)
    ref = FR.feature_cos(h.numpy(), r.numpy(), frames, gs, T)
    d_ref, l_ref = ref["dist"], ref["loss"]
    fr = [int(v) for v in ref["frames"]]
    out = _call(h, r, frames, H, gs)
    assert out["status"] == _lib.PAA_OK
    # two calls give the same bits; dist and dh are nullable and do not change the loss
    again = _call(h, r, frames, H, gs)
    assert same_bits(out["loss"], again["loss"]) and same_bits(out["dist"], again["dist"]) and same_bits(out["dh"], again["dh"])
    bare = _call(h, r, frames, H, gs, dist=False, dh=False)
    assert bare["status"] == _lib.PAA_OK and same_bits(bare["loss"], out["loss"])
    only_d = _call(h, r, frames, H, gs, dh=False)
    assert same_bits(only_d["loss"], out["loss"]) and same_bits(only_d["dist"], out["dist"])
    # rows past T_b and the pad rows of dh, and the frames past T_b of dist, are exact zeros (the buffers held a sentinel)
    for b in range(B):
        assert (out["dh"][b, fr[b]:].view(np.uint32) == 0).all() and (out["dist"][b, fr[b]:].view(np.uint32) == 0).all(), b
    # the degenerate rows: d = 1 and a zero cotangent row, exactly
    live = np.zeros((B, T), bool)
    for b in range(B):
        live[b, :fr[b]] = True
    for b, t in (DEG_H, DEG_R):
        if live[b, t]:
            assert out["dist"][b, t] == 1.0 and d_ref[b, t] == 1.0 and (out["dh"][b, t].view(np.uint32) == 0).all(), (b, t)
    # the yardstick: torch float32 on the CPU, the same function of the same inputs (the degenerate rows carry ordinary values there
    # and are left out of the comparison: they were checked exactly above)
    h32, r32 = h[:, :T].clone(), r.clone()
    h32[DEG_H], r32[DEG_R] = 1.0, 1.0
    ht = h32.requires_grad_(True)
    keep = torch.from_numpy(live)
    d_t = (1.0 - F.cosine_similarity(ht, r32, dim=-1, eps=0.0)) * keep
    (gs * d_t.sum()).backward()
    ok = live.copy()
    ok[DEG_H], ok[DEG_R] = False, False
    dh_ref = ref["dh"][:, :T]
    b_dh = row_bound(dh_ref, ht.grad.numpy())                       # (B, T): one bound per cotangent row
    e_dh = row_err(out["dh"][:, :T], dh_ref)
    o_dh = over(e_dh, b_dh)[ok]
    # d: every frame is a row of one value; the torch error is taken per frame, the floor from the value itself
    e_d = np.abs(out["dist"].astype(np.float64) - d_ref)
    b_d = row_bound(d_ref[..., None], d_t.detach().numpy()[..., None])
    o_d = over(e_d, b_d)[ok]
    # loss_b: the B clips as one row, against torch's float32 sum over the frames (a degenerate frame contributes its 1 there too)
    l_t = torch.where(torch.from_numpy(live & ~ok), torch.ones(()), d_t.detach()).sum(dim=1).numpy()
    e_l = np.abs(out["loss"].astype(np.float64) - l_ref)
    b_l = row_bound(l_ref, l_t)
    print(f"H {H} frames {frames}: dh err {e_dh[ok].max():.3e} (torch f32 {row_err(ht.grad.numpy(), dh_ref)[ok].max():.3e}, worst "
          f"err / bound {o_dh.max():.3f}); d err {e_d[ok].max():.3e} (torch f32 "
          f"{np.abs(d_t.detach().numpy() - d_ref)[ok].max():.3e}, worst {o_d.max():.3f}); loss err {e_l.max():.3e} (torch f32 "
          f"{np.abs(l_t - l_ref).max():.3e}, worst {over(e_l, b_l).max():.3f})")
    assert o_dh.max() <= 1.0 and o_d.max() <= 1.0 and over(e_l, b_l).max() <= 1.0
    assert np.abs(dh_ref[ok]).max() > 0 and d_ref[NEAR] < 1e-3 and np.isfinite(out["dh"]).all() and np.isfinite(out["dist"]).all()
    # the entry's two roundings, restated: d once, the loss from the float64 sum of the rounded d
    d32, l32 = FR.rounded(ref)
    assert np.allclose(out["loss"], l32, rtol=LOSS_RTOL, atol=0)


def test_feature_distance_wrapper_and_unaligned_rows():
    """core.features.feature_distance on dense tensors, and the dword path of the kernel (an operand that is not 16-byte aligned)
    against the 16-byte path: the same bits."""
    H = 72
    h, r = _cos_inputs(H)
    hd, rd = h[:, :T].contiguous().cuda(), r.cuda()
    loss, dist, dh = core_features.feature_distance(hd, rd, [24, 7, 1], grad=True, grad_scale=2.0)
    ref = FR.feature_cos(h[:, :T].numpy(), r.numpy(), [24, 7, 1], 2.0)
    d32, l32 = FR.rounded(ref)
    assert np.allclose(loss.cpu().numpy(), l32, rtol=LOSS_RTOL, atol=0) and rel_err(dist.cpu().numpy(), d32) < 1e-6
    assert rel_err(dh.cpu().numpy(), ref["dh"]) < 1e-6
    l2, d2 = core_features.feature_distance(hd, rd, [24, 7, 1])
    assert torch.equal(l2, loss) and torch.equal(d2, dist)
    # shift h by one float: its rows stay H floats long but start 4 bytes off the 16-byte grid
    buf = torch.zeros(hd.numel() + 1, device="cuda")
    buf[1:] = hd.reshape(-1)
    Lb = _lib.lib()
    out_l, out_dh = torch.empty(B, device="cuda"), torch.empty_like(hd)
    work = torch.empty(int(Lb.paa_feature_cos_work_floats(B, T)), device="cuda")
    fr = torch.tensor([24, 7, 1], dtype=torch.int32, device="cuda")
    assert Lb.paa_feature_cos(buf.data_ptr() + 4, T, _lib.ptr(rd), T, _lib.ptr(fr), B, T, H, 2.0, _lib.ptr(out_l), None, _lib.ptr(out_dh),
                              _lib.ptr(work), _lib.stream_ptr()) == _lib.PAA_OK
    torch.cuda.synchronize()
    assert torch.equal(out_l, loss) and torch.equal(out_dh, dh)


def test_feature_cos_refusals():
    Lb = _lib.lib()
    H = 64
    h, r = torch.zeros(B, H_ROWS, H, device="cuda"), torch.zeros(B, T, H, device="cuda")
    loss, dh = torch.zeros(B, device="cuda"), torch.zeros(B, H_ROWS, H, device="cuda")
    work = torch.zeros(int(Lb.paa_feature_cos_work_floats(B, T)) + 4, device="cuda")
    p = _lib.ptr

    def call(h_=h, r_=r, loss_=loss, work_=p(work), H_=H, h_rows=H_ROWS, ref_rows=T):
        return Lb.paa_feature_cos(None if h_ is None else p(h_), h_rows, None if r_ is None else p(r_), ref_rows, None, B, T, H_, 1.0,
                                  None if loss_ is None else p(loss_), None, p(dh), work_, _lib.stream_ptr())

    assert call() == _lib.PAA_OK
    assert call(h_=None) == ARG and call(r_=None) == ARG and call(loss_=None) == ARG and call(work_=None) == ARG
    assert call(work_=work.data_ptr() + 4) == ARG                      # a misaligned work buffer
    assert call(H_=6) == SIZE and call(H_=4100) == SIZE and call(H_=0) == SIZE
    assert call(h_rows=T - 1) == SIZE and call(ref_rows=T - 1) == SIZE
    torch.cuda.synchronize()


# ================================================================================ the hidden state's way out ===
def _oracle_hidden(sd, a, x):
    """The oracle's last hidden state: feature encoder, feature projection, encoder (oracle/wav2vec2.py), composed as logits_of
    composes them, without lm_head."""
    f = OW.feature_encoder(sd, a, x).transpose(1, 2)
    f = F.layer_norm(f, (f.shape[-1],), sd["wav2vec2.feature_projection.layer_norm.weight"],
                     sd["wav2vec2.feature_projection.layer_norm.bias"], eps=a.layer_norm_eps)
    h = F.linear(f, sd["wav2vec2.feature_projection.projection.weight"], sd["wav2vec2.feature_projection.projection.bias"])
    return OW.encoder(sd, a, h)


def _inputs():
    clean = torch.from_numpy(synth.clean_audio(B, L))
    p = torch.from_numpy(synth.perturbation(L).reshape(1, L) * np.float32(1e-2))
    rows = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * 1e-2)
    return clean, p, rows


def _padded(m, name, cols, nb=B):
    return m.debug_read(name, nb).reshape(nb, m.layout(-1), cols)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["group", "layer"])
def test_features_vs_oracle(variant, dtype):
    a = _arch(variant)
    sdn = A.rule_weights(a)
    sd = OW.to_torch(sdn)
    clean, p, rows = _inputs()
    m = PaaModel(a, sdn, B, L, dtype)
    with pytest.raises(KeyError):
        m.debug_read("hfinal", B)                      # the f32 hidden buffer does not exist before the first use
    H = a.hidden_size
    for name, pert, x in (("clean", None, clean), ("universal", p, (clean + p).clamp(-1, 1)), ("rows", rows, (clean + rows).clamp(-1, 1))):
        got = m.features(clean.cuda(), None if pert is None else pert.cuda())
        torch.cuda.synchronize()
        with torch.no_grad():
            ref = _oracle_hidden(sd, a, x)
        e = rel_err(got.cpu().numpy(), ref.numpy())
        print(f"{variant} {dtype} {name}: last hidden state rel err {e:.3e} (bound {ACT_TOL[dtype]})")
        assert tuple(got.shape) == (B, T, H) == tuple(ref.shape) and e < ACT_TOL[dtype], (name, e)
        assert same_bits(_padded(m, "hfinal", H)[:, :T], got.cpu().numpy())
    # the unclamped sum, as the evaluation composes it
    big = clean * 15
    got = m.features(big.cuda(), p.cuda(), clamp=False)
    with torch.no_grad():
        ref = _oracle_hidden(sd, a, big + p)
    assert rel_err(got.cpu().numpy(), ref.numpy()) < ACT_TOL[dtype]
    # the logits of a training call are those of a model that never produced features
    fresh = PaaModel(a, sdn, B, L, dtype)
    labels = opgd.make_labels(["ab cd", "hello", "ab"], cli_to_args("snr", []), B)
    r1, r2 = m.fwd_bwd(clean.cuda(), p.cuda(), labels, +1), fresh.fwd_bwd(clean.cuda(), p.cuda(), labels, +1)
    torch.cuda.synchronize()
    assert torch.equal(r1["logits"], r2["logits"]) and torch.equal(r1["grad"], r2["grad"]) and torch.equal(r1["stats"], r2["stats"])


@pytest.mark.parametrize("variant", ["group", "layer"])
def test_features_true_clip_lengths(variant):
    a = _arch(variant, hd64=True)
    clean, p, rows = _inputs()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    m.set_lengths([8000, 6400, 4800])
    frames = m.frame_counts(B).cpu().tolist()
    assert frames == [24, 19, 14]
    got = m.features(clean.cuda(), rows.cuda()).cpu().numpy()
    for b, tb in enumerate(frames):
        assert (got[b, tb:].view(np.uint32) == 0).all() and np.abs(got[b, :tb]).max(axis=1).min() > 0 and np.isfinite(got[b]).all(), b
    # the loss under lengths: frames past T_b carry neither loss nor cotangent
    ref = torch.zeros(B, T, a.hidden_size, device="cuda")
    m.features(clean.cuda(), None, out=ref)
    m.set_feature_loss(ref)
    r = m.fwd_bwd(clean.cuda(), rows.cuda(), None, +1)
    torch.cuda.synchronize()
    fr = FR.feature_cos(_padded(m, "hfinal", a.hidden_size), ref.cpu().numpy(), frames, 1.0, T)
    _, l32 = FR.rounded(fr)
    assert np.allclose(m.debug_read("nll", B), l32, rtol=LOSS_RTOL, atol=0) and (l32 > 0).all()
    assert abs(float(r["stats"][0]) - float(l32.astype(np.float64).sum())) <= LOSS_RTOL * float(l32.sum())
    assert torch.isfinite(r["grad"]).all() and float(r["grad"].abs().max()) > 0


# ================================================================================ the loss inside fwd_bwd ===
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["group", "layer"])
def test_loss_stats_and_input_gradient(variant, dtype):
    a = _arch(variant)
    sdn = A.rule_weights(a)
    sd = OW.to_torch(sdn)
    clean, p, rows = _inputs()
    m = PaaModel(a, sdn, B, L, dtype)
    H = a.hidden_size
    ref = m.features(clean.cuda()).contiguous()
    m.set_feature_loss(ref)
    ref_np = ref.cpu().numpy()
    for name, pert in (("universal", p), ("rows", rows)):
        r = m.fwd_bwd(clean.cuda(), pert.cuda(), None, +1)
        torch.cuda.synchronize()
        fr = FR.feature_cos(_padded(m, "hfinal", H), ref_np, None, 1.0, T)
        _, l32 = FR.rounded(fr)
        total = float(l32.astype(np.float64).sum())
        print(f"{variant} {dtype} {name}: stats[0] {float(r['stats'][0])!r} reference {total!r} per clip {l32.tolist()}")
        assert (l32 > 0).all() and np.abs(fr["dh"]).sum() > 0
        assert abs(float(r["stats"][0]) - total) <= LOSS_RTOL * total
        assert np.allclose(m.debug_read("nll", B), l32, rtol=LOSS_RTOL, atol=0)
        # the oracle's autograd with the reference's cotangent injected at the hidden state
        pr = pert.clone().requires_grad_(True)
        hid = _oracle_hidden(sd, a, (clean + pr).clamp(-1, 1))
        hid.backward(gradient=torch.from_numpy(fr["dh"][:, :T].astype(np.float32)))
        e = rel_err(r["grad"].cpu().numpy(), pr.grad.numpy())
        print(f"{variant} {dtype} {name}: grad rel err {e:.3e} (bound {GRAD_TOL[dtype]})")
        assert r["grad"].shape == pr.grad.shape and e < GRAD_TOL[dtype], (name, e)
        # the logits are produced as ever
        with torch.no_grad():
            lg = OW.logits_of(sd, a, (clean + pert).clamp(-1, 1))
        assert rel_err(r["logits"].cpu().numpy(), lg.numpy()) < ACT_TOL[dtype]
    # direction is the grad_scale: -1 flips the gradient (the backward pass is linear in its cotangent, so the two differ by the
    # rounding of the bf16 planes alone: far inside the gradient's own tolerance) and leaves the loss
    rd = m.fwd_bwd(clean.cuda(), rows.cuda(), None, +1)
    rn = m.fwd_bwd(clean.cuda(), rows.cuda(), None, -1)
    torch.cuda.synchronize()
    e = rel_err(rn["grad"].cpu().numpy(), -rd["grad"].cpu().numpy())
    print(f"{variant} {dtype}: direction -1 against the negated +1 gradient {e:.2e}")
    assert e < GRAD_TOL[dtype] / 10 and torch.equal(rn["stats"][0], rd["stats"][0])
    # every clip's row is the gradient of its solo run (the solo call reads row 0 of the reference)
    for b in range(B):
        solo_ref = torch.zeros_like(ref)
        solo_ref[0] = ref[b]
        m.set_feature_loss(solo_ref)
        r1 = m.fwd_bwd(clean[b:b + 1].cuda(), rows[b:b + 1].cuda(), None, +1)
        torch.cuda.synchronize()
        e = rel_err(rd["grad"][b].cpu().numpy(), r1["grad"][0].cpu().numpy())
        el = abs(float(r1["stats"][0]) - float(m.debug_read("nll", 1)[0]))
        print(f"{variant} {dtype}: clip {b} row vs its solo run {e:.2e} (bit-equal {torch.equal(rd['grad'][b], r1['grad'][0])})")
        assert e < 1e-5 and el == 0.0, (b, e)
    m.set_feature_loss(ref)
    # a call without a gradient reports the feature loss too; labels are not read; paa_model_forward keeps reporting CTC
    labels = opgd.make_labels(["ab cd", "hello", "ab"], cli_to_args("snr", []), B)
    ng = m.fwd_bwd(clean.cuda(), rows.cuda(), None, +1, want_grad=False)
    wl = m.fwd_bwd(clean.cuda(), rows.cuda(), labels, +1)
    fw = m.forward(clean.cuda(), rows.cuda(), labels, clamp=True)
    torch.cuda.synchronize()
    assert torch.equal(ng["loss"], rd["loss"]) and torch.equal(wl["loss"], rd["loss"]) and torch.equal(wl["grad"], rd["grad"])
    m.set_feature_loss(None)
    ctc = m.fwd_bwd(clean.cuda(), rows.cuda(), labels, +1, want_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(fw["loss"], ctc["loss"]) and not torch.equal(ctc["loss"], rd["loss"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["group", "layer"])
def test_zero_perturbation_has_zero_distance(variant, dtype):
    a = _arch(variant)
    clean, _, _ = _inputs()
    m = PaaModel(a, A.rule_weights(a), B, L, dtype)
    ref = m.features(clean.cuda()).contiguous()
    m.set_feature_loss(ref)
    for rows_ in (B, 1):
        r = m.fwd_bwd(clean.cuda(), torch.zeros(rows_, L, device="cuda"), None, +1)
        torch.cuda.synchronize()
        # first: the hidden state of clamp(clean + 0) IS the reference, bit for bit ...
        assert same_bits(_padded(m, "hfinal", a.hidden_size)[:, :T], ref.cpu().numpy())
        # ... then every dot product of a frame is the same double, so d is a rounding of 1 - s / (sqrt(s) sqrt(s))
        nll = m.debug_read("nll", B)
        print(f"{variant} {dtype} p = 0 ({rows_} rows): loss per clip {nll.tolist()}")
        assert (np.abs(nll) <= T * 2.0 ** -40).all() and abs(float(r["stats"][0])) <= B * T * 2.0 ** -40
        assert torch.isfinite(r["grad"]).all()


# ================================================================================ switching off ===
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_switching_off_restores_the_bits_of_a_fresh_model(dtype):
    a = _arch("group")
    sdn = A.rule_weights(a)
    clean, p, rows = _inputs()
    labels = opgd.make_labels(["ab cd", "hello", "ab"], cli_to_args("snr", []), B)
    m, fresh = PaaModel(a, sdn, B, L, dtype), PaaModel(a, sdn, B, L, dtype)
    # without the feature loss a gradient still needs labels
    with pytest.raises(Exception, match="gradient requested without labels"):
        m.fwd_bwd(clean.cuda(), p.cuda(), None, +1)
    ref = m.features(clean.cuda()).contiguous()
    m.set_feature_loss(ref)
    assert m.feature_ref is ref
    m.fwd_bwd(clean.cuda(), p.cuda(), None, +1)
    m.set_feature_loss(None)
    assert m.feature_ref is None
    for pert in (p, rows):
        r, f = m.fwd_bwd(clean.cuda(), pert.cuda(), labels, +1), fresh.fwd_bwd(clean.cuda(), pert.cuda(), labels, +1)
        torch.cuda.synchronize()
        assert torch.equal(r["grad"], f["grad"]) and torch.equal(r["logits"], f["logits"]) and torch.equal(r["stats"], f["stats"])
        assert same_bits(m.debug_read("dlogits", B), fresh.debug_read("dlogits", B))
    with pytest.raises(Exception, match="gradient requested without labels"):
        m.fwd_bwd(clean.cuda(), p.cuda(), None, +1)
    # mutually exclusive with the alignment-margin loss, in both orders
    m.set_loss(1, 1.0)
    with pytest.raises(_lib.PaaError, match="alignment-margin loss is active"):
        m.set_feature_loss(ref)
    assert m.feature_ref is None and m.loss_kind == 1
    m.set_loss(0)
    m.set_feature_loss(ref)
    with pytest.raises(_lib.PaaError, match="feature-distance loss is active"):
        m.set_loss(1, 1.0)
    assert m.loss_kind == 0 and m.feature_ref is ref
    m.set_loss(0)                                      # kind 0 is no conflict
    with pytest.raises(Exception, match="kind"):
        m.set_loss(2, 1.0)
    # a reference of another shape, dtype or device is refused on the host
    for bad in (ref[:, :-1], ref.double(), ref.cpu(), ref.transpose(1, 2)):
        with pytest.raises(ValueError, match="feature reference"):
            m.set_feature_loss(bad)
    m.set_feature_loss(None)


# ================================================================================ the device steps ===
def _args(norm="snr", flags=("--snr_db", "10", "--lr", "0.01"), feature=True):
    args = cli_to_args(norm, list(flags))
    args.device = "cuda"
    if feature:
        args.loss_type = "feature"
    return args


def _hand_steps(m, args, x0, clean, n, rows):
    """n steps sequenced by hand on a model of its own: features, fwd_bwd, sign step, projection."""
    Lb = _lib.lib()
    x = x0.clone()
    nb = clean.shape[0]
    ref = torch.zeros(m.max_batch, m.frames, m.arch.hidden_size, device="cuda")
    m.set_feature_loss(ref)
    proj = runtime.get_proj(args, m.device, nb if rows else 1, L, None)
    prm = runtime.params_of(args, "snr")
    losses = []
    for i in range(n):
        if not rows or i == 0:                          # the universal step recomputes the reference, the per-clip step keeps it
            m.features(clean, None, out=ref)
        r = m.fwd_bwd(clean, x, None, +1)
        losses.append(r["stats"][0].clone())
        st = _lib.stream_ptr()
        _lib.check(Lb.paa_sign_step(_lib.ptr(x), _lib.ptr(r["grad"]), float(args.lr), x.numel(), st))
        if rows:
            _lib.check(Lb.paa_project_rows(proj.h, prm, _lib.ptr(x), _lib.ptr(x), nb, _lib.ptr(clean), L, st))
        else:
            _lib.check(Lb.paa_project(proj.h, prm, _lib.ptr(x), 1, _lib.ptr(clean), nb, L, st))
    torch.cuda.synchronize()
    return x, losses


@pytest.mark.parametrize("kind", ["clip", "universal"])
def test_steps_equal_hand_sequence_and_replay(kind):
    a = _arch("group")
    sdn = A.rule_weights(a)
    args = _args()
    clean, p, rows = _inputs()
    clean = clean.cuda()
    labels = opgd.make_labels(["ab cd", "hello", "ab"], args, B)
    m, hand = PaaModel(a, sdn, B, L, "fp32"), PaaModel(a, sdn, B, L, "fp32")
    if kind == "clip":
        st, x0, lab = ClipStepper(m, args, L), rows.cuda(), None          # the step reads no labels: None is allowed
        with pytest.raises(RuntimeError, match="feature_reset"):
            st.step(x0.clone(), clean, lab)
        st.feature_reset(clean)
    else:
        st, x0, lab = PgdStepper(m, args, L), p.cuda(), labels
    assert m.feature_ref is st.feat_ref and st.direction == +1 and st.modes.feature_on
    xh, losses_h = _hand_steps(hand, args, x0, clean, 2, kind == "clip")
    xe = x0.clone()
    losses = []
    for _ in range(2):
        r = st.step(xe, clean, lab)
        losses.append(r["loss"].clone())
    torch.cuda.synchronize()
    print(f"{kind}: feature loss over two eager steps {[float(v) for v in losses]}")
    assert torch.equal(xe, xh) and all(torch.equal(u, v) for u, v in zip(losses, losses_h)) and not torch.equal(xe, x0)
    assert float(losses[0]) > 0
    # captured replay equals eager, bit for bit
    xg, cbuf = x0.clone(), clean.clone()
    g, rg = st.capture(xg, cbuf, lab)
    xg.copy_(x0)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(xg, xe) and torch.equal(rg["loss"], losses[-1])
    if kind == "universal":
        # a replay on a second clean batch: the reference is recomputed inside the graph
        clean2 = torch.from_numpy(synth.clean_audio(B, L, seed=11)).cuda()
        assert not torch.equal(clean2, clean)
        cbuf.copy_(clean2)
        xg.copy_(x0)
        g.replay()
        torch.cuda.synchronize()
        loss_g = rg["loss"].clone()
        assert torch.equal(st.feat_ref, hand.features(clean2))
        x2 = x0.clone()
        r2 = st.step(x2, clean2, lab)
        torch.cuda.synchronize()
        assert torch.equal(xg, x2) and torch.equal(loss_g, r2["loss"])
    # a CTC stepper on the same model sets the model back before its own step
    ctc = ClipStepper(m, _args(feature=False), L)
    ctc.step(rows.cuda(), clean, labels)
    assert m.feature_ref is None and m.loss_kind == 0


def test_clip_step_with_adam_and_true_clip_lengths():
    """The per-clip step under Adam in the length mode: the reference is taken after the lengths are set, the loss in the stats slot
    is the reference's on the model's own hidden state over T_b frames, the tail of every row stays zero, and the captured step
    replays to the eager bits."""
    a = _arch("group", hd64=True)
    args = _args("linf", ("--linf_size", "0.05", "--lr", "0.002"))
    clean, _, rows = _inputs()
    clean, lens = clean.cuda(), [8000, 6400, 4800]
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")

    def run(replay):
        x = rows.cuda().clone()
        for b, n in enumerate(lens):
            x[b, n:] = 0.0
        st = ClipStepper(m, args, L, optimizer=torch.optim.Adam([x], lr=args.lr))
        st.set_lengths(lens)
        st.feature_reset(clean)
        if replay:
            g, r = st.capture(x, clean, None)
            for _ in range(2):
                g.replay()
        else:
            for _ in range(2):
                r = st.step(x, clean, None)
        torch.cuda.synchronize()
        return x, r["loss"].clone(), st

    xe, le, st = run(False)
    frames = m.frame_counts(B).cpu().tolist()
    assert frames == [24, 19, 14]
    fr = FR.feature_cos(_padded(m, "hfinal", a.hidden_size), st.feat_ref.cpu().numpy(), frames, 1.0, T)
    total = float(FR.rounded(fr)[1].astype(np.float64).sum())
    assert total > 0 and abs(float(le) - total) <= LOSS_RTOL * total
    for b, n in enumerate(lens):
        assert not xe[b, n:].any() and xe[b, :n].any() and not torch.equal(xe[b, :n], rows.cuda()[b, :n])
    xg, lg, _ = run(True)
    assert torch.equal(xg, xe) and torch.equal(lg, le)
    m.set_lengths(None)


def test_universal_step_with_the_masking_loss_term():
    """The masking-threshold loss term rides along: slot 6 holds it, slot 0 the feature distance, and the gradient is the feature
    gradient minus alpha times the term's (paa_masking_loss subtracts in place after the backward pass)."""
    a = _arch("group")
    sdn = A.rule_weights(a)
    clean, p, _ = _inputs()
    clean = clean.cuda()
    plain, masked = _args(), _args()
    masked.masking_loss_alpha = 0.5
    m1, m2 = PaaModel(a, sdn, B, L, "fp32"), PaaModel(a, sdn, B, L, "fp32")
    s1, s2 = PgdStepper(m1, plain, L), PgdStepper(m2, masked, L)
    x1, x2 = p.cuda().clone(), p.cuda().clone()
    r1, r2 = s1.step(x1, clean, None), s2.step(x2, clean, None)
    torch.cuda.synchronize()
    assert torch.equal(r1["loss"], r2["loss"]) and float(r2["masking_loss"]) > 0 and float(s1.stats[6]) == 0.0
    assert not torch.equal(s1.grad, s2.grad) and torch.isfinite(s2.grad).all() and torch.isfinite(x2).all()


def test_steppers_refuse_targeted_and_eot():
    a = _arch("group")
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    args = _args()
    args.attack_mode, args.target, args.target_reps = "targeted", "ab", 1
    for make in (ClipStepper, PgdStepper):
        with pytest.raises(ValueError, match="does not run with --attack_mode targeted"):
            make(m, args, L)
    args = _args()
    args.place_gain_db = 6.0
    with pytest.raises(NotImplementedError, match="not implemented with --eot_draws"):
        ClipStepper(m, args, L, eot_draws=2)
    assert m.feature_ref is None


# ================================================================================ the runners ===
def test_runners_end_to_end(tmp_path):
    logs = str(tmp_path / "clips")
    args = attack_clips.create_arg_parser().parse_args(
        ["--arch", "tiny", "--device", "cuda", "--audio_seconds", "0.5", "--batch_size", "4", "--steps_per_epoch", "2", "--small_data",
         "--silent", "--norm_type", "snr", "--snr_db", "20", "--pgd_steps", "2", "--optimizer_type", "pgd", "--lr", "1e-3",
         "--num_items_to_inspect", "0", "--dtype", "fp32", "--loss_type", "feature", "--logs_dir", logs])
    assert attack_clips.main(args) == 0
    assert "_feature" in os.path.basename(args.save_dir)
    res = json.load(open(os.path.join(args.save_dir, "clip_results.json")))
    assert res["loss_type"] == "feature" and len(res["clips"]) >= 2 and res["summary"]["clips"] == len(res["clips"])
    for c in res["clips"]:
        assert set(attack_clips.RECORD_FIELDS) <= set(c) and np.isfinite(c["final_ctc"]) and c["l2"] > 0
    rargs = parser.create_arg_parser().parse_args(
        ["--arch", "tiny", "--audio_seconds", "0.5", "--batch_size", "4", "--steps_per_epoch", "2", "--num_epochs", "1", "--logs_dir",
         str(tmp_path / "run"), "--dtype", "fp32", "--silent", "--optimizer_type", "pgd", "--norm_type", "snr", "--snr_db", "20",
         "--loss_type", "feature"])
    assert run_attack.main(rargs) == 0
    assert "_feature" in os.path.basename(rargs.save_dir)
    d = json.load(open(os.path.join(rargs.save_dir, "results.json")))
    assert d["finished_training"] == 1.0 and d["loss_type"] == "feature" and "final_test_perturbed" in d
    # the training field named ctc holds the feature distance: a sum of cosine distances, within [0, 2] per frame
    assert 0.0 < d["best_train_score"]["ctc"] <= 2.0 * 4 * T
    # --attack_mode targeted is refused with the rule's message
    targ = parser.create_arg_parser().parse_args(
        ["--arch", "tiny", "--norm_type", "snr", "--optimizer_type", "pgd", "--attack_mode", "targeted", "--loss_type", "feature",
         "--logs_dir", str(tmp_path / "t"), "--silent"])
    with pytest.raises(ValueError, match="--loss_type feature does not run with --attack_mode targeted"):
        run_attack.main(targ)
    targ = attack_clips.create_arg_parser().parse_args(
        ["--arch", "tiny", "--norm_type", "snr", "--optimizer_type", "pgd", "--attack_mode", "targeted", "--loss_type", "feature",
         "--logs_dir", str(tmp_path / "t2"), "--silent"])
    with pytest.raises(ValueError, match="--loss_type feature does not run with --attack_mode targeted"):
        attack_clips.main(targ)
