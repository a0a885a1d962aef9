"""-m gpu: the masking norm (clean-signal frequency-masking threshold) against tests/masking_ref.py: the
threshold entry point, the projection (per clip and universal), composites, the device steps and the runners."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import masking_ref as MR
from gpu_util import rel_err
from oracle import pgd as opgd, wav2vec2 as OW
from oracle.gen_cases import PGD_TEXTS, cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.core.masking import masking_threshold
from paa_amd.model import PaaModel
from paa_amd.training_utils import train
from paa_amd.training_utils.clip_attack import ClipStepper
from paa_amd.training_utils.pgd import PgdStepper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


def _args(margin=0.0, norm="masking"):
    a = cli_to_args(norm, ["--masking_margin_db", str(margin)] if margin else [])
    a.masking_margin_db = float(margin)
    a.device = "cuda"
    return a


def _tone(k, L, amp):
    return (amp * np.sin(2 * np.pi * k * np.arange(L) / 1024.0)).astype(np.float32)


def _inputs():
    """(name, (B, L) float32) cases: speech-like clips, tones, silence, a zero-padded tail and lengths off the hop grid."""
    cases = [("synth_3x10s", synth.clean_audio(3, 160000))]
    L = 16000
    cases.append(("tones", np.stack([_tone(64, L, 0.5), _tone(64, L, 0.5) + _tone(66, L, 0.3),
                                     _tone(40, L, 0.2) + _tone(50, L, 0.2) + _tone(63, L, 0.2) + _tone(200, L, 0.05)])))
    cases.append(("zero", np.zeros((1, 8737), np.float32)))
    tail = synth.clean_audio(1, 16000)
    tail[:, 9000:] = 0.0
    cases.append(("zero_tail", tail))
    for L in (4096, 5000, 16000, 8737, 10250):
        cases.append((f"L{L}", synth.clean_audio(2, L, seed=7)))
    return cases


def test_threshold_vs_reference():
    args = _args()
    frames_ok = frames_all = 0
    for name, x in _inputs():
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        theta, pmax, pbar = masking_threshold(xd, args, psd=True)
        theta2, pmax2 = masking_threshold(xd, args)
        torch.cuda.synchronize()
        assert torch.equal(theta, theta2) and torch.equal(pmax, pmax2), name        # deterministic
        th, pm, pb = theta.cpu().numpy(), pmax.cpu().numpy(), pbar.cpu().numpy()
        for b in range(x.shape[0]):
            P, pmax_ref = MR.levels(x[b])
            mag_ref = np.abs(MR.stft_tf(x[b]))
            assert abs(pm[b] - pmax_ref) < 1e-4, (name, b, pm[b], pmax_ref)
            mag_dev = np.sqrt(np.maximum(10.0 ** ((pb[b].astype(np.float64) - 96.0 + pm[b]) / 10.0) - 1e-20, 0.0))
            assert np.abs(mag_dev - mag_ref).max() <= 2e-5 * max(mag_ref.max(), 1e-30), name
            th_ref, margin, nsurv, _ = MR.threshold_from_pbar(pb[b], SR)
            ok = margin >= 1e-4
            both_inf = np.isneginf(th_ref) & np.isneginf(th[b])
            with np.errstate(invalid="ignore"):
                diff = np.where(both_inf, 0.0, np.abs(th[b].astype(np.float64) - th_ref))
            bad = ok & (diff.max(axis=1) > 0.01)
            assert not bad.any(), (name, b, np.nonzero(bad)[0][:5], diff[ok].max())
            frames_ok += int(ok.sum())
            frames_all += ok.size
            print(f"{name}[{b}]: pmax {pm[b]:.3f} dB, max |dtheta| {diff[ok].max() if ok.any() else 0:.2e} dB over "
                  f"{ok.sum()}/{ok.size} frames, maskers/frame {nsurv.mean():.1f}")
    assert frames_ok >= 0.99 * frames_all, (frames_ok, frames_all)


def test_zero_clip_is_ath():
    args = _args()
    theta, pmax = masking_threshold(torch.zeros(2, 4096, device="cuda"), args)
    z, q, ath, kA, _, _ = MR.tables(SR)
    th = theta.cpu().numpy()
    assert np.isneginf(th[:, :, :kA]).all()
    np.testing.assert_allclose(th[:, :, kA:], np.broadcast_to(ath[kA:], th[:, :, kA:].shape), atol=1e-3)


def _rows_case(B, L, seed=3, amp=1e-2):
    clean = synth.clean_audio(B, L, seed=seed)
    d = (np.stack([synth.normal(synth.key_of(f"mask{b}", seed), L) for b in range(B)]) * amp).astype(np.float32)
    return clean, d


def _proj_rows(pr, prm, src, clean, out=None):
    B, L = src.shape
    out = torch.empty_like(src) if out is None else out
    _lib.check(_lib.lib().paa_project_rows(pr.h, prm, _lib.ptr(src), _lib.ptr(out), B, _lib.ptr(clean), L, _lib.stream_ptr()))
    return out


@pytest.mark.parametrize("margin", [0.0, -6.0])
def test_project_rows_vs_reference(margin):
    args = _args(margin)
    prm = runtime.params_of(args)
    for B, L in ((3, 16000), (2, 8737), (2, 10250)):
        clean_np, d_np = _rows_case(B, L)
        clean, d = torch.from_numpy(clean_np).cuda(), torch.from_numpy(d_np).cuda()
        pr = runtime.get_proj(args, d.device, B, L)
        got = _proj_rows(pr, prm, d, clean)
        inplace = d.clone()
        _proj_rows(pr, prm, inplace, clean, out=inplace)
        theta, pmax = masking_threshold(clean, args)
        torch.cuda.synchronize()
        assert torch.equal(inplace, got)
        th, pm, g = theta.cpu().numpy(), pmax.cpu().numpy(), got.cpu().numpy()
        for b in range(B):
            ref = MR.project(d_np[b], MR.bound(th[b], pm[b], margin), L)
            e = np.abs(g[b] - ref).max() / np.abs(ref).max()
            assert e < 2e-5, (B, L, b, e)
            assert np.abs(ref - d_np[b]).max() > 1e-3 * np.abs(d_np[b]).max()        # the bound is active
            one = torch.empty_like(d[b:b + 1])
            _lib.check(_lib.lib().paa_project_to(pr.h, prm, _lib.ptr(d[b:b + 1].contiguous()), _lib.ptr(one), 1,
                                                 _lib.ptr(clean[b:b + 1].contiguous()), 1, L, _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(one[0], got[b]), (B, L, b)                          # row == the one-row call


def test_under_bound_unchanged_and_zero():
    args = _args()
    prm = runtime.params_of(args)
    B, L = 2, 16000
    clean_np, _ = _rows_case(B, L)
    clean = torch.from_numpy(clean_np).cuda()
    theta, pmax = masking_threshold(clean, args)
    th, pm = theta.cpu().numpy(), pmax.cpu().numpy()
    d_np = (clean_np * 1e-7).astype(np.float32)
    for b in range(B):        # precondition: every bin of delta lies under the bound
        assert (np.abs(MR.stft_tf(d_np[b])) <= MR.bound(th[b], pm[b])).all()
    pr = runtime.get_proj(args, clean.device, B, L)
    got = _proj_rows(pr, prm, torch.from_numpy(d_np).cuda(), clean).cpu().numpy()
    valid = 256 * (L // 256)
    assert np.abs(got[:, :valid] - d_np[:, :valid]).max() <= 1e-6 * np.abs(d_np).max()
    assert (got[:, valid:] == 0).all()
    zero = _proj_rows(pr, prm, torch.zeros(B, L, device="cuda"), clean)
    assert (zero == 0).all()


def test_universal_vs_reference_and_composite():
    args = _args()
    prm = runtime.params_of(args)
    B, L = 3, 16000
    clean_np, d_np = _rows_case(B, L)
    clean, d = torch.from_numpy(clean_np).cuda(), torch.from_numpy(d_np[:1]).cuda()
    pr = runtime.get_proj(args, d.device, B, L)
    out = torch.empty_like(d)
    _lib.check(_lib.lib().paa_project_to(pr.h, prm, _lib.ptr(d), _lib.ptr(out), 1, _lib.ptr(clean), B, L, _lib.stream_ptr()))
    inplace = d.clone()
    _lib.check(_lib.lib().paa_project(pr.h, prm, _lib.ptr(inplace), 1, _lib.ptr(clean), B, L, _lib.stream_ptr()))
    theta, pmax = masking_threshold(clean, args)
    torch.cuda.synchronize()
    assert torch.equal(out, inplace)
    th, pm = theta.cpu().numpy(), pmax.cpu().numpy()
    A_min = np.min(np.stack([MR.bound(th[b], pm[b]) for b in range(B)]), axis=0)
    ref = MR.project(d_np[0], A_min, L)
    assert np.abs(out.cpu().numpy()[0] - ref).max() < 2e-5 * np.abs(ref).max()
    # the public constraint: the same, and masking+l2 == masking then l2
    q = train.perturbation_constraint(d, clean, args, None, None)
    assert torch.equal(q, out)
    args2 = _args(norm="masking+l2")
    args2.l2_size = 0.01
    both = train.perturbation_constraint(d, clean, args2, None, None)
    a_l2 = types.SimpleNamespace(**{**vars(args2), "norm_type": "l2"})
    seq = train.perturbation_constraint(out, clean, a_l2, None, None)
    torch.cuda.synchronize()
    assert torch.equal(both, seq)
    with pytest.raises(ValueError):
        train.perturbation_constraint(d, None, args, None, None)


def test_errors():
    args = _args()
    prm = runtime.params_of(args)
    pr = runtime.get_proj(args, "cuda", 1, 4096)
    d = torch.zeros(1, 4096, device="cuda")
    st = _lib.lib().paa_project(pr.h, prm, _lib.ptr(d), 1, None, 0, 4096, _lib.stream_ptr())
    assert st == _lib.PAA_ERR_NEED_CLEAN
    stats = torch.zeros(2, device="cuda")
    st = _lib.lib().paa_project_ext(pr.h, prm, _lib.ptr(d), 1, _lib.ptr(stats), None, 4096.0, 4096, _lib.stream_ptr())
    assert st == _lib.PAA_ERR_BAD_NORM
    S = torch.zeros(1, 17, 513, 2, device="cuda")
    st = _lib.lib().paa_spectrum_project(pr.h, prm, _lib.ptr(S), _lib.ptr(S), 1, 17, _lib.stream_ptr())
    assert st == _lib.PAA_ERR_BAD_NORM
    odd = types.SimpleNamespace(**{**vars(args), "n_fft": 512, "win_length": 512, "hop_length": 128})
    pr2 = runtime.get_proj(odd, "cuda", 1, 4096)
    st = _lib.lib().paa_project(pr2.h, prm, _lib.ptr(d), 1, _lib.ptr(d), 1, 4096, _lib.stream_ptr())
    assert st == _lib.PAA_ERR_ARG


def _model(variant, B, L):
    a = A.tiny() if variant == "group" else A.tiny("layer", stable=True)
    sdn = A.rule_weights(a)
    return a, sdn, PaaModel(a, sdn, B, L, "fp32")


@pytest.mark.parametrize("variant", ["group", "layer"])
@pytest.mark.parametrize("opt", ["pgd", "adam"])
def test_clip_step_equals_universal_batch1_and_replay(variant, opt):
    B, L = 2, 8737
    args = _args()
    args.lr = 1e-3
    a, sdn, m = _model(variant, B, L)
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    d0 = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"m{b}", 5), L) for b in range(B)]).astype(np.float32) * 1e-2).cuda()
    de = torch.nn.Parameter(d0.clone())
    opt_c = torch.optim.Adam([de], lr=args.lr) if opt == "adam" else None
    st = ClipStepper(m, args, L, optimizer=opt_c)
    for _ in range(2):
        st.step(de.data, clean, labels)
    torch.cuda.synchronize()
    m1 = PaaModel(a, sdn, 1, L, "fp32")
    for b in range(B):
        pb = torch.nn.Parameter(d0[b:b + 1].clone())
        opt_u = torch.optim.Adam([pb], lr=args.lr) if opt == "adam" else None
        su = PgdStepper(m1, args, L, optimizer=opt_u)
        for _ in range(2):
            su.step(pb.data, clean[b:b + 1].contiguous(), labels[b:b + 1])
        torch.cuda.synchronize()
        assert torch.equal(pb.data[0], de.data[b]), (variant, opt, b)
    if opt == "pgd":      # eager == captured replay, both steppers
        dg = d0.clone()
        g, r = st.capture(dg, clean, labels)
        dg.copy_(d0)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dg, de.data)
        su = PgdStepper(m, args, L)
        pe = d0[:1].clone()
        for _ in range(2):
            su.step(pe, clean, labels)
        pg = d0[:1].clone()
        g2, _ = su.capture(pg, clean, labels)
        pg.copy_(d0[:1])
        for _ in range(2):
            g2.replay()
        torch.cuda.synchronize()
        assert torch.equal(pg, pe)


def test_universal_step_vs_oracle():
    B, L = 2, 16000
    args = _args()
    a = A.tiny()
    sdn = A.rule_weights(a)
    clean = torch.from_numpy(synth.clean_audio(B, L))
    p0 = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2))
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    a_lin = types.SimpleNamespace(**{**vars(args), "norm_type": "linf", "linf_size": 1e9})
    ref = opgd.pgd_step(OW.to_torch(sdn), a, a_lin, clean, labels, p0)
    m = PaaModel(a, sdn, B, L, "fp32")
    st = PgdStepper(m, args, L)
    p = p0.cuda()
    r = st.step(p, clean.cuda(), labels)
    theta, pmax = masking_threshold(clean.cuda(), args)
    torch.cuda.synchronize()
    g, gref = st.grad.cpu().numpy()[0], ref["grad"].numpy()[0]
    assert rel_err(g, gref) < 5e-3 and float((np.sign(g) != np.sign(gref)).mean()) < 5e-3
    assert abs(float(r["loss"]) - float(ref["loss"])) < 2e-4 * abs(float(ref["loss"]))
    th, pm = theta.cpu().numpy(), pmax.cpu().numpy()
    A_min = np.min(np.stack([MR.bound(th[b], pm[b]) for b in range(B)]), axis=0)
    pexp = MR.project(p0.numpy()[0] + args.lr * np.sign(g), A_min, L)
    e_p = np.abs(p.cpu().numpy()[0] - pexp).max() / np.abs(pexp).max()
    assert e_p < 5e-5, e_p


def test_attack_clips_entry_point(tmp_path):
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, "-m", "paa_amd.attack_clips", "--arch", "tiny", "--device", "cuda", "--audio_seconds", "0.5",
           "--batch_size", "2", "--steps_per_epoch", "1", "--small_data", "--silent", "--norm_type", "masking",
           "--pgd_steps", "3", "--optimizer_type", "pgd", "--num_items_to_inspect", "2", "--logs_dir", logs]
    assert subprocess.run(cmd, cwd=ROOT, timeout=600).returncode == 0
    found = [os.path.join(d, "clip_results.json") for d, _, fs in os.walk(logs) if "clip_results.json" in fs]
    assert found
    res = json.load(open(found[0]))
    assert all(np.isfinite(c["final_ctc"]) for c in res["clips"])


def test_run_attack_one_rank(tmp_path):
    cmd = [sys.executable, "-m", "paa_amd.run_attack", "--arch", "tiny", "--audio_seconds", "0.5", "--batch_size", "2",
           "--steps_per_epoch", "1", "--num_epochs", "1", "--logs_dir", str(tmp_path), "--dtype", "fp32", "--silent",
           "--optimizer_type", "pgd", "--norm_type", "masking"]
    assert subprocess.run(cmd, cwd=ROOT, timeout=600).returncode == 0
