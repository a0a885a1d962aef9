"""-m gpu: true clip lengths through the model, the steppers and the per-clip entry point, against the
float64 restatement tests/varlen_ref.py (pinned to HuggingFace with an attention_mask by tests/test_varlen_host.py).

The tiny architectures run with head dim 64 (test_gpu_model.HD64): only the fused attention path supports lengths.  Bounds are
the ones tests/test_gpu_model.py applies to the tiny architectures for the same dtype: ACT_TOL on loss and logits, GRAD_TOL on the
waveform gradient (test_tiny_intermediates, which runs these very architectures in both dtypes); sign flips below 5e-3 in fp32
(test_pgd_step_vs_reference_goldens, the tiny goldens).  No tiny-architecture test of that file asserts a bf16 sign-flip rate: the
bf16 bound here, 0.03, is the tightest one its bf16 step tests apply (test_full_size_bf16_vs_fp32_parity and
test_full_size_base_16x30s: 0.03; test_full_size_large_lv60_32x10s: 0.05)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import varlen_ref as VR
from gpu_util import rel_err
from oracle import pgd as opgd, wav2vec2 as OW
from oracle.gen_cases import PGD_TEXTS, cli_to_args
from paa_amd import _lib, arch as A, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils import build
from paa_amd.training_utils.clip_attack import ClipStepper
from paa_amd.training_utils.pgd import PgdStepper
from test_gpu_model import ACT_TOL, GRAD_TOL, HD64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 8000
LENGTH_SETS = {"a": [8000, 5321, 3000], "b": [8000, 400, 4321]}
FLIP_TOL = {"fp32": 5e-3, "bf16": 0.03}
VARIANTS = ["group", "layer_stable"]


def arch_of(variant):
    return A.tiny("group", False, **HD64) if variant == "group" else A.tiny("layer", True, **HD64)


def texts_for(a, lengths):
    return [("a" if t < 8 else PGD_TEXTS[b]) for b, t in enumerate(VR.frame_counts(a, lengths))]


def inputs(a, lengths):
    B = len(lengths)
    clean = torch.from_numpy(synth.clean_audio(B, L)) * VR.sample_mask(lengths, L, torch.float32)
    p = torch.from_numpy(synth.perturbation(L).reshape(1, L) * np.float32(1e-2))
    rows = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * 1e-2)
    args = cli_to_args("snr", ["--snr_db", "40"])
    args.device = "cuda"
    return clean, p, rows, opgd.make_labels(texts_for(a, lengths), args, B), args


_ref = {}


def reference(variant, key):
    """float64 reference of the universal and of the per-row step, computed once per (variant, length set)."""
    if (variant, key) not in _ref:
        a, lengths = arch_of(variant), LENGTH_SETS[key]
        clean, p, rows, labels, _ = inputs(a, lengths)
        sd = {k: v.double() for k, v in OW.to_torch(A.rule_weights(a)).items()}
        uni = VR.step_reference(sd, a, clean.double(), p.double(), labels, lengths)
        per = VR.step_reference(sd, a, clean.double(), rows.double(), labels, lengths, rows=True)
        _ref[variant, key] = (uni, per)
    return _ref[variant, key]


@pytest.mark.parametrize("key", list(LENGTH_SETS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_model_vs_reference(variant, dtype, key):
    a, lengths = arch_of(variant), LENGTH_SETS[key]
    B, frames = len(lengths), VR.frame_counts(a, lengths)
    clean, p, rows, labels, _ = inputs(a, lengths)
    m = PaaModel(a, A.rule_weights(a), B, L, dtype)
    m.set_lengths(lengths)
    assert m.frame_counts(B).cpu().tolist() == frames
    blank = a.pad_token_id
    for form, pert, (l_ref, lg_ref, g_ref) in zip(("universal", "rows"), (p, rows), reference(variant, key)):
        r = m.fwd_bwd(clean.cuda(), pert.cuda(), labels, +1)
        torch.cuda.synchronize()
        lg, g = r["logits"].cpu().numpy(), r["grad"].cpu().numpy()
        lg_ref, g_ref = lg_ref.numpy(), g_ref.numpy().reshape(g.shape)
        e_loss = abs(float(r["loss"]) - l_ref) / abs(l_ref)
        e_lg = max(np.abs(lg[b, :t] - lg_ref[b, :t]).max() for b, t in enumerate(frames)) / np.abs(lg_ref).max()
        e_g = rel_err(g, g_ref)
        flips = float((np.sign(g) != np.sign(g_ref)).mean())
        print(f"VARLEN {variant} {dtype} {key} {form}: loss {e_loss:.2e} logits {e_lg:.2e} grad {e_g:.2e} flips {flips:.2e}")
        assert np.isfinite(l_ref) and e_loss < ACT_TOL[dtype] and e_lg < ACT_TOL[dtype], (form, e_loss, e_lg)
        assert e_g < GRAD_TOL[dtype] and flips < FLIP_TOL[dtype], (form, e_g, flips)
        ids = loss_helpers.argmax_ids(r["logits"], m.frame_counts(B), blank).cpu().numpy()
        for b, t in enumerate(frames):
            assert not lg[b, t:].any(), (form, b, "logits rows >= T_b must be zero")
            assert (ids[b, t:] == blank).all(), (form, b)
            assert np.array_equal(ids[b, :t], lg[b, :t].argmax(-1)), (form, b)
        if form == "rows":
            for b, n in enumerate(lengths):
                assert not g[b, n:].any() and np.abs(g[b, :n]).max() > 0, (b, "gradient beyond len_b must be exactly 0")
        else:
            assert not g[0, max(lengths):].any()
    # forward-only entry: the same logits, and the loss of the clamped composition
    fw = m.forward(clean.cuda(), rows.cuda(), labels, clamp=True)
    assert torch.equal(fw["logits"], r["logits"]) and torch.equal(fw["loss"], r["loss"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_universal_gradient_is_exactly_zero_beyond_every_clip(variant, dtype):
    """The sum-over-clips form (k_input_grad<false> / k_input_grad_gn<false>) with EVERY clip shorter than L: no clip contributes
    beyond max_b len_b, so the universal gradient there is exactly 0 — with the GroupNorm extractor an unmasked gradient is
    non-zero up to the last sample (through the time statistics).  Below each clip's end the row-sum still has terms."""
    a, lengths = arch_of(variant), [7000, 400, 4321]
    B = len(lengths)
    clean, p, _, labels, _ = inputs(a, lengths)
    m = PaaModel(a, A.rule_weights(a), B, L, dtype)
    m.set_lengths(lengths)
    r = m.fwd_bwd(clean.cuda(), p.cuda(), labels, +1)
    torch.cuda.synchronize()
    g = r["grad"].cpu().numpy()
    assert g.shape == (1, L) and np.isfinite(g).all() and np.isfinite(float(r["loss"]))
    assert (g[0, max(lengths):] == 0).all(), np.abs(g[0, max(lengths):]).max()
    # every segment between two clip ends still receives the longer clips' terms
    for lo, hi in ((0, 400), (400, 4321), (4321, 7000)):
        assert np.abs(g[0, lo:hi]).max() > 0, (lo, hi)
    # the same clips against a clean batch that is NOT zero beyond the clips' ends: the mask is the kernels', not the input's
    full = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    r2 = m.fwd_bwd(full, p.cuda(), labels, +1)
    torch.cuda.synchronize()
    assert torch.equal(r2["grad"], r["grad"]) and torch.equal(r2["loss"], r["loss"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_full_lengths_agree_with_lengths_off(variant, dtype):
    a = arch_of(variant)
    B = 3
    clean, p, _, labels, _ = inputs(a, [L] * B)
    m = PaaModel(a, A.rule_weights(a), B, L, dtype)
    off = m.fwd_bwd(clean.cuda(), p.cuda(), labels, +1)
    off = {k: off[k].clone() for k in ("loss", "logits", "grad")}
    m.set_lengths([L] * B)
    on = m.fwd_bwd(clean.cuda(), p.cuda(), labels, +1)
    torch.cuda.synchronize()
    assert abs(float(on["loss"]) - float(off["loss"])) < ACT_TOL[dtype] * abs(float(off["loss"]))
    assert rel_err(on["logits"].cpu().numpy(), off["logits"].cpu().numpy()) < ACT_TOL[dtype]
    assert rel_err(on["grad"].cpu().numpy(), off["grad"].cpu().numpy()) < GRAD_TOL[dtype]
    m.set_lengths(None)                      # off again: the bits of a model that never had lengths
    again = m.fwd_bwd(clean.cuda(), p.cuda(), labels, +1)
    torch.cuda.synchronize()
    assert all(torch.equal(again[k], off[k]) for k in off)


def test_lengths_are_validated_and_need_fused_attention():
    a = arch_of("group")
    m = PaaModel(a, A.rule_weights(a), 3, L, "fp32")
    for bad in ([399, 8000, 8000], [8000, 8001, 500], [8000.0, 500.0, 500.0], [8000] * 4):
        with pytest.raises(ValueError):
            m.set_lengths(bad)
    assert not m.lengths_on
    small = A.tiny()                           # head dim 16: materialised attention
    ms = PaaModel(small, A.rule_weights(small), 2, L, "fp32")
    with pytest.raises(_lib.PaaError) as e:
        ms.set_lengths([8000, 4000])
    assert e.value.status == _lib.PAA_ERR_ARG and not ms.lengths_on


@pytest.mark.parametrize("opt", ["pgd", "adam"])
@pytest.mark.parametrize("norm", ["snr", "max_phon"])
def test_clip_stepper_replay_equals_eager_and_follows_the_buffer(norm, opt):
    """Eager == captured-and-replayed, bit for bit; a new length buffer between replays changes the step without re-capture;
    delta_b[len_b:] is zero after every step."""
    a = arch_of("group")
    la, lb = LENGTH_SETS["a"], LENGTH_SETS["b"]
    B = len(la)
    clean, _, rows, _, _ = inputs(a, [L] * B)
    labels = inputs(a, lb)[3]                  # feasible at both length sets (one token for the one-frame clip)
    args = cli_to_args(norm, ["--snr_db", "40"] if norm == "snr" else [])
    args.device = "cuda"
    args.lr = 1e-3
    spl = build.init_phon_threshold_tensor(args)
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean, d0 = clean.cuda(), rows.cuda()

    def stepper(d):
        o = torch.optim.Adam([d], lr=args.lr) if opt == "adam" else None
        return ClipStepper(m, args, L, None, spl, optimizer=o)

    def tails_zero(d, lengths):
        return all(not d[b, n:].any().item() for b, n in enumerate(lengths))

    de = torch.nn.Parameter(d0.clone()) if opt == "adam" else d0.clone()
    se = stepper(de)
    for lengths in (la, la, lb):
        se.step(de.data, clean, labels, lengths=lengths)
        assert tails_zero(de.data, lengths)
    d_a = d0.clone()                           # what two more steps at the FIRST lengths would have given
    dg = torch.nn.Parameter(d0.clone()) if opt == "adam" else d0.clone()
    sg = stepper(dg)
    g, r = sg.capture(dg.data, clean, labels, lengths=la)
    dg.data.copy_(d0)
    for _ in range(2):
        g.replay()
        assert tails_zero(dg.data, la)         # after every replayed step
    sg.set_lengths(lb)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(dg.data, de.data) and torch.isfinite(de.data).all().item()
    assert tails_zero(dg.data, lb) and torch.isfinite(r["loss"]).item()
    with pytest.raises(ValueError):
        sg.set_lengths(None)                   # the captured sequence runs in the length mode
    # the third step did depend on the buffer: three steps at the first lengths end elsewhere
    sa = stepper(torch.nn.Parameter(d_a)) if opt == "adam" else stepper(d_a)
    for _ in range(3):
        sa.step(d_a, clean, labels, lengths=la)
    torch.cuda.synchronize()
    assert not torch.equal(d_a, de.data)
    m.set_lengths(None)


def test_universal_stepper_replay_follows_the_buffer():
    a = arch_of("layer_stable")
    la, lb = LENGTH_SETS["a"], LENGTH_SETS["b"]
    B = len(la)
    clean, p0, _, _, args = inputs(a, [L] * B)
    labels = inputs(a, lb)[3]                  # feasible at both length sets
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean, p0 = clean.cuda(), p0.cuda()
    st = PgdStepper(m, args, L)
    pe = p0.clone()
    for lengths in (la, lb):
        st.step(pe, clean, labels, lengths=lengths)
    pg = p0.clone()
    g, _ = st.capture(pg, clean, labels, lengths=la)
    pg.copy_(p0)
    g.replay()
    st.set_lengths(lb)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pg, pe) and torch.isfinite(pe).all().item()


def test_stepper_refuses_what_lengths_do_not_support():
    a = arch_of("group")
    B = 3
    clean, p0, _, labels, _ = inputs(a, [L] * B)
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    for norm, extra in (("masking", []), ("snr", ["--masking_loss_alpha", "0.5"]), ("snr", ["--place_shift", "random"]),
                        ("snr", ["--rir_bank", "synthetic"])):
        args = cli_to_args(norm, extra)
        args.device = "cuda"
        with pytest.raises(ValueError, match="--clip_lengths"):
            PgdStepper(m, args, L).step(p0.cuda(), clean.cuda(), labels, lengths=LENGTH_SETS["a"])
        assert not m.lengths_on


def test_attack_clips_record_equals_the_clip_alone():
    """attack_batch at B = 3 under lengths against the same clip attacked alone at the same L.  Index, length and the WERs are
    compared exactly.  The float fields (CTC losses, norms, SNR) are held to 1e-5 relative, the bound
    test_gpu_clip_attack.test_entry_point_two_ranks_equal_one applies to the same fields across batch splits: bit equality across
    batch sizes is not part of the GEMMs' contract (their tile selection depends on the row count M = B * P, and torch's row
    reductions on the shape).  The worst difference is printed; DESIGN.md section 6h records the measured figure."""
    from paa_amd import attack_clips as AC
    a = arch_of("group")
    lengths = LENGTH_SETS["a"]
    B = len(lengths)
    clean, _, _, _, _ = inputs(a, lengths)
    args = AC.create_arg_parser().parse_args(["--norm_type", "snr", "--snr_db", "40", "--pgd_steps", "3", "--clip_lengths", "true"])
    args.device = "cuda"
    texts = texts_for(a, lengths)
    x = clean.cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    recs, delta, adv, _ = AC.attack_batch(m, None, args, x, texts, [10, 11, 12], None, None, None, torch.tensor(lengths))
    assert [r["length"] for r in recs] == lengths
    worst, same_delta = 0.0, True
    for b, n in enumerate(lengths):
        assert not delta[b, n:].any() and not adv[b, n:].any() and np.isfinite(recs[b]["final_ctc"])
        one, d1, _, _ = AC.attack_batch(m, None, args, x[b:b + 1], texts[b:b + 1], [10 + b], None, None, None,
                                        torch.tensor(lengths[b:b + 1]))
        assert one[0]["index"] == recs[b]["index"] and one[0]["length"] == n
        assert one[0]["clean_wer"] == recs[b]["clean_wer"] and one[0]["adv_wer"] == recs[b]["adv_wer"]
        for k in ("clean_ctc", "final_ctc", "l2", "linf", "snr_db"):
            worst = max(worst, abs(one[0][k] - recs[b][k]) / max(abs(recs[b][k]), 1e-6))
            assert abs(one[0][k] - recs[b][k]) <= 1e-5 * max(abs(recs[b][k]), 1e-6), (b, k, one[0][k], recs[b][k])
        same_delta &= torch.equal(d1[0], delta[b])
    print(f"VARLEN attack_clips B=3 vs alone: worst relative difference of a float field {worst:.2e}; delta rows bit-equal: {same_delta}")
    m.set_lengths(None)


def test_two_ranks_equal_one_under_lengths(tmp_path):
    import varlen_dist_child as child
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "varlen_dist_child.py"),
                               str(r), "2", str(port), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for r in range(2)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=330))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    res = []
    for pr, (so, se) in zip(procs, outs):
        assert pr.returncode == 0, (so[-2000:], se[-4000:])
        res.append(json.loads([l for l in so.splitlines() if l.startswith("VARLEN_CHILD ")][-1][len("VARLEN_CHILD "):]))
    assert all(d["replicas_identical"] for d in res), res
    p_dp = np.load(tmp_path / "rank0.npz")["p"]
    a, args, B = arch_of("group"), child.case_args(), 2
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    p = torch.from_numpy(synth.perturbation(L).reshape(1, L) * np.float32(1e-2)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    st = PgdStepper(m, args, L)
    for _ in range(child.STEPS):
        r = st.step(p, clean, opgd.make_labels(child.TEXTS, args, B), lengths=list(child.LENGTHS))
    torch.cuda.synchronize()
    assert res[0]["loss"] == pytest.approx(float(r["loss"]), rel=1e-5)
    diff = np.abs(p_dp - p.cpu().numpy())
    scale = np.abs(p.cpu().numpy()).max()
    print(f"lengths DP vs single max diff {diff.max() / scale:.2e}; fraction differing {(diff > 1e-6 * scale).mean():.2e}")
    assert (diff > 1e-5 * scale).mean() < 5e-3          # only where a gradient sign is numerically undecided


def test_train_epoch_and_evaluate_pass_lengths_through():
    """train_epoch and evaluate on (x, texts, lengths) batches, on the host-WER and the device-WER route: the two routes give
    the same perturbation and scores, and the epoch's loss is the loss of a step taken by hand under the same lengths."""
    from paa_amd.training_utils import evaluation, parser, train
    a = arch_of("group")
    texts = ["ab cd", "a", "hello"]
    lens = [torch.tensor([8000, 400, 4321], dtype=torch.int32), torch.tensor([5321, 3000, 8000], dtype=torch.int32)]
    x = torch.from_numpy(synth.clean_audio(3, L))
    batches = [(build.zero_tails(x.clone(), ln), texts, ln) for ln in lens]
    p0 = torch.from_numpy(synth.perturbation(L).reshape(1, L) * np.float32(1e-2)).cuda()
    m = PaaModel(a, A.rule_weights(a), 3, L, "fp32")
    out = {}
    for route in ("host", "device"):
        args = parser.create_arg_parser().parse_args(["--norm_type", "snr", "--snr_db", "40", "--clip_lengths", "true",
                                                      "--batch_size", "3", "--optimizer_type", "pgd", "--device", "cuda"]
                                                     + (["--device_wer"] if route == "device" else []))
        res = train.train_epoch(args, batches, p0.clone(), m, 0, None, None, None, None, None)
        assert m.lengths_on
        sc = evaluation.evaluate(args, batches, res.p, m, None, None, perturbed=True)
        out[route] = (res, sc)
        assert np.isfinite(res.avg_ctc) and np.isfinite(sc.ctc) and 0 <= sc.wer and 0 <= res.avg_wer
    (rh, sh), (rd, sd_) = out["host"], out["device"]
    assert torch.equal(rh.p, rd.p)
    assert rh.avg_ctc == pytest.approx(rd.avg_ctc, rel=1e-6) and rh.avg_wer == pytest.approx(rd.avg_wer, abs=1e-12)
    assert sh.ctc == pytest.approx(sd_.ctc, rel=1e-6) and sh.wer == pytest.approx(sd_.wer, abs=1e-12)
    # by hand: the same two steps under the same lengths
    args = cli_to_args("snr", ["--snr_db", "40"])
    args.device = "cuda"
    st = PgdStepper(m, args, L)
    p, losses = p0.clone(), []
    for xb, tb, ln in batches:
        r = st.step(p, xb.cuda(), opgd.make_labels(tb, args, 3), lengths=ln)
        losses.append(float(r["loss"]))
    assert torch.equal(p, rh.p)
    assert rh.avg_ctc == pytest.approx(sum(losses) / len(losses), rel=1e-6)
    # padded mode afterwards switches the model's length mode off again
    args.clip_lengths = "padded"
    evaluation.evaluate(args, [(xb, tb) for xb, tb, _ in batches], p, m, None, None, perturbed=True)
    assert not m.lengths_on
