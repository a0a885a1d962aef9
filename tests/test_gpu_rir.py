"""-m gpu: room responses on the placement layer — paa_rir_apply in both directions and paa_rir_draw against
tests/rir_ref.py, the step with the mode on against the oracle, the draw inside captured graphs, the mode off, Adam on a short
perturbation, two ranks, evaluation and the runner.

Bounds.  paa_rir_apply is one f32 fmaf chain per output over at most K + 38 terms, of which at most K are not exact zeros:
|dev - ref64| <= (K + 64) 2^-24 sum_k |h_k x| + 2^-149 per output (rir_ref.bound; derived, not calibrated).  The step bounds are
those of test_gpu_place.test_placed_step_vs_oracle.  Every kernel output lives between two guard blocks that must survive."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import place_ref as PR
import rir_ref as RR
from gpu_util import record_launches, rel_err
from oracle import pgd as opgd, projections as OP, wav2vec2 as OW
from oracle.gen_cases import PGD_TEXTS, cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.model import PaaModel
from paa_amd.training_utils import build, place, rir
from paa_amd.training_utils.pgd import PgdStepper
from test_gpu_place import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, L, K, N, index): distinct, repeated and out-of-range (reduced modulo N) indices
APPLY_CASES = [(1, 1, 1, 1, [0]), (2, 257, 1, 3, [2, -1]), (3, 1000, 7, 3, [1, 1, 5]), (2, 300, 512, 2, [1, 0]),
               (2, 4099, 1024, 3, [2, 3]), (4, 5000, 4096, 3, [0, 2, 2, -2]), (1, 2048, 16384, 2, [3])]


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    """max_phon contours are loaded into the process-wide projection contexts: drop them for the modules that follow."""
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def _bank(N, K, tag="bank"):
    """Asymmetric responses: decaying normals, nothing palindromic."""
    h = synth.normal(synth.key_of(f"{tag}{N}x{K}", 5), N * K).reshape(N, K) * np.exp(-np.arange(K) / max(K / 3.0, 1.0))
    return h.astype(np.float32)


def _signal(B, L, tag):
    return np.stack([synth.normal(synth.key_of(f"{tag}{b}_{L}", 5), L) for b in range(B)]).astype(np.float32)


def _apply(bank, index, x, adjoint):
    """One paa_rir_apply launch between guard blocks -> the (B, L) output tensor."""
    B, L = x.shape
    N, K = bank.shape
    out = Guarded((B, L))
    _lib.check(_lib.lib().paa_rir_apply(_lib.ptr(bank), N, K, _lib.ptr(index), _lib.ptr(x), out.ptr, B, L, adjoint, _lib.stream_ptr()))
    torch.cuda.synchronize()
    out.check()
    return out.t


# ---- 1. paa_rir_apply, both directions -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,K,N,index", APPLY_CASES)
def test_rir_apply_vs_float64(B, L, K, N, index):
    bank_np, x_np, g_np = _bank(N, K), _signal(B, L, "x"), _signal(B, L, "g")
    bank, idx = torch.from_numpy(bank_np).cuda(), _i32(index)
    outs = {}
    for adjoint, src in ((0, x_np), (1, g_np)):
        d = torch.from_numpy(src).cuda()
        a = _apply(bank, idx, d, adjoint)
        b = _apply(bank, idx, d, adjoint)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                 # two calls: the same bits
        dev = a.cpu().numpy().astype(np.float64)
        ref = (RR.adjoint64 if adjoint else RR.apply64)(bank_np, index, src)
        bound = RR.bound(bank_np, index, src, bool(adjoint))
        err = np.abs(dev - ref)
        print(f"B={B} L={L} K={K} adjoint={adjoint}: max err / bound {float((err / bound).max()):.4f}, max |ref| {np.abs(ref).max():.3g}")
        assert np.isfinite(dev).all() and np.all(err <= bound), float((err / bound).max())
        outs[adjoint] = (dev, bound)
    # <apply(x), G> = <x, adjoint(G)>, in float64 on the device outputs, within the sum of the two bounds
    x64, g64 = x_np.astype(np.float64), g_np.astype(np.float64)
    lhs, rhs = math.fsum((outs[0][0] * g64).ravel()), math.fsum((x64 * outs[1][0]).ravel())
    tol = math.fsum((outs[0][1] * np.abs(g64)).ravel()) + math.fsum((np.abs(x64) * outs[1][1]).ravel())
    print(f"B={B} L={L} K={K}: adjointness |lhs - rhs| / tol {abs(lhs - rhs) / tol:.4f}")
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


@pytest.mark.parametrize("L", [1, 257, 4096, 4097, 20001])
def test_identity_and_pure_delay_are_exact(L):
    """K = 1, h = [1]: the input; h = e_d: the input d samples later with zeros in front (adjoint: d samples earlier, zeros
    behind) — exact, every product is 1 * x or 0 * x.  4096 / 4097 straddle one block's span, 20001 needs five blocks."""
    B = 2
    x_np = _signal(B, L, "id")
    x = torch.from_numpy(x_np).cuda()
    one = torch.ones(1, 1, device="cuda")
    for adjoint in (0, 1):
        assert torch.equal(_apply(one, _i32([0, 0]), x, adjoint), x)
    for K, d in ((5, 4), (40, 33), (2150, 2100)):            # d past one tile row, and past one staged chunk of the response
        bank_np = np.zeros((2, K), dtype=np.float32)
        bank_np[0, d], bank_np[1, 0] = 1.0, 1.0             # row 1 is the identity
        bank = torch.from_numpy(bank_np).cuda()
        want = np.zeros_like(x_np)
        want[0, d:] = x_np[0, :max(L - d, 0)]
        want[1] = x_np[1]
        assert np.array_equal(_apply(bank, _i32([0, 1]), x, 0).cpu().numpy(), want), (L, K, d)
        want = np.zeros_like(x_np)
        want[0, :max(L - d, 0)] = x_np[0, d:]
        want[1] = x_np[1]
        assert np.array_equal(_apply(bank, _i32([0, 1]), x, 1).cpu().numpy(), want), (L, K, d)


def test_rir_refusals_leave_outputs_alone():
    L_ = _lib.lib()
    B, L, N, K = 2, 600, 3, 16
    bank, x, idx = torch.zeros(N, K, device="cuda"), torch.zeros(B, L, device="cuda"), _i32([0, 1])
    out, index, counter = Guarded((B, L)), Guarded((B,), torch.int32), Guarded((1,), torch.int32)
    st, ARG = _lib.stream_ptr(), _lib.PAA_ERR_ARG
    for N_, K_, B_, L__ in ((0, K, B, L), (N, 0, B, L), (N, 16385, B, L), (N, K, 0, L), (N, K, B, 0)):
        for adjoint in (0, 1):
            assert L_.paa_rir_apply(_lib.ptr(bank), N_, K_, _lib.ptr(idx), _lib.ptr(x), out.ptr, B_, L__, adjoint, st) == ARG
    for k in range(3):
        a = [_lib.ptr(bank), _lib.ptr(idx), _lib.ptr(x)]
        a[k] = None
        assert L_.paa_rir_apply(a[0], N, K, a[1], a[2], out.ptr, B, L, 0, st) == ARG
    assert L_.paa_rir_apply(_lib.ptr(bank), N, K, _lib.ptr(idx), _lib.ptr(x), None, B, L, 0, st) == ARG
    assert L_.paa_rir_apply(_lib.ptr(bank), N, K, _lib.ptr(idx), out.ptr, out.ptr, B, L, 0, st) == ARG          # in place
    assert b"overlap" in L_.paa_last_error()
    half = Guarded((2 * B, L))
    assert L_.paa_rir_apply(_lib.ptr(bank), N, K, _lib.ptr(idx), half.ptr, _lib.ptr(half.t[1:]), B, L, 1, st) == ARG
    with pytest.raises(_lib.PaaError, match="overlap"):
        _lib.check(L_.paa_rir_apply(_lib.ptr(bank), N, K, _lib.ptr(idx), _lib.ptr(half.t[1:]), half.ptr, B, L, 0, st))
    assert L_.paa_rir_draw(5, None, 0, 0, B, N, index.ptr, st) == ARG
    assert L_.paa_rir_draw(5, counter.ptr, 0, 0, B, N, None, st) == ARG
    assert L_.paa_rir_draw(5, counter.ptr, 0, 0, 0, N, index.ptr, st) == ARG
    assert L_.paa_rir_draw(5, counter.ptr, 0, 0, B, 0, index.ptr, st) == ARG
    torch.cuda.synchronize()
    for g in (out, half, index, counter):
        g.check()
        assert g.untouched()


# ---- 2. paa_rir_draw -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 64])
def test_rir_draw(N):
    for B in (5, 1, 257):          # 257: one past the block, the draw's clip loop takes a second pass
        _rir_draw(N, B)


def _rir_draw(N, B):
    base, seed = 7, 5
    counter = Guarded((1,), torch.int32)
    counter.t.zero_()
    for step in range(3):
        index = Guarded((B,), torch.int32)
        _lib.check(_lib.lib().paa_rir_draw(seed, counter.ptr, 0, base, B, N, index.ptr, _lib.stream_ptr()))
        torch.cuda.synchronize()
        index.check(), counter.check()
        assert index.t.cpu().tolist() == RR.draw(seed, step, base, B, 0, N).tolist(), step
        assert int(counter.t.item()) == step + 1                 # one per launch, not one per clip
    if N == 64:          # the evaluation stream, another seed and placement's counter word draw other rooms
        index = Guarded((B,), torch.int32)
        counter.t.zero_()
        _lib.check(_lib.lib().paa_rir_draw(seed + (1 << 32), counter.ptr, 1, base, B, N, index.ptr, _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = index.t.cpu().tolist()
        assert got == RR.draw(seed + (1 << 32), 0, base, B, 1, N).tolist() and got != RR.draw(seed, 0, base, B, 0, N).tolist()
        assert RR.draw(seed, 0, base, B, 0, N).tolist() != [PR.draw_shift(seed, 0, base + b, 0, N) for b in range(B)]


# ---- 3. the step with the mode on against the oracle ---------------------------------------------------------------------
#            norm, extra, Lp (None: placement off), shifts, gains, rooms
STEP_CASES = {"alone": ("linf", [], None, (0, 0), None, (1, 2)),
              "shift_gain": ("snr", ["--snr_db", "40"], 16000, (5555, 143), (0.7, 1.3), (2, 2)),
              "short": ("max_phon", [], 4096, (12, 4095), None, (0, 4))}
STEP_N, STEP_K = 3, 600


@pytest.mark.parametrize("variant", ["group", "layer"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_reverberant_step_vs_oracle(case, variant):
    norm, extra, Lp, shifts, gains, rooms = STEP_CASES[case]
    a = A.tiny("group", False) if variant == "group" else A.tiny("layer", True)
    B, L = 2, 16000
    args = cli_to_args(norm, extra)
    args.device, args.sr, args.seed = "cuda", 16000, 5
    args.rir_bank, args.rir_count, args.rir_taps = "synthetic", STEP_N, STEP_K
    if Lp is not None:
        args.perturbation_seconds = Lp / 16000
    Lp = L if Lp is None else Lp
    bank_np = rir.bank_of(args)
    assert bank_np.shape == (STEP_N, STEP_K)
    sdn = A.rule_weights(a)
    sd = OW.to_torch(sdn)
    clean = torch.from_numpy(synth.clean_audio(B, L))
    p0 = torch.from_numpy(synth.perturbation(Lp) * np.float32(1e-3)).view(1, Lp)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    spl = OP.spl_thresh_tensor(args)
    m = PaaModel(a, sdn, B, L, "fp32")
    st = PgdStepper(m, args, L, None, build.init_phon_threshold_tensor(args))
    assert st.rir_on and st.place_on == (case != "alone") and st.Lp == Lp and st.packed.numel() == Lp + 8
    assert st.placer.rows.shape == (B, L) and st.reverb.rows.shape == (B, L) and st.reverb.grad_rows.shape == (B, L)
    if st.place_on:
        st.set_placement(shifts, gains)
    else:
        with pytest.raises(RuntimeError):
            st.set_placement(shifts)
    st.set_rooms(rooms)
    p = p0.cuda()
    r = st.step(p, clean.cuda(), labels)
    torch.cuda.synchronize()
    g = st.grad.cpu().numpy()[0]
    g32 = None if gains is None else np.asarray(gains, dtype=np.float32)
    rows0 = PR.place(p0.numpy()[0], L, shifts, g32)
    assert torch.equal(st.placer.rows.cpu(), torch.from_numpy(rows0))
    wet64 = RR.apply64(bank_np, rooms, rows0)                                    # the rows convolved in numpy float64 first
    wet_dev = st.reverb.rows.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(wet_dev - wet64) <= RR.bound(bank_np, rooms, rows0))
    ref = opgd.pgd_step(sd, a, args, clean, labels, torch.from_numpy(wet64.astype(np.float32)), spl)
    gref = PR.reduce64(RR.adjoint64(bank_np, rooms, ref["grad"].numpy()), shifts, g32, Lp)[0]        # and the adjoint in numpy
    e_g = rel_err(g, gref)
    flips = float((np.sign(g) != np.sign(gref)).mean())
    e_loss = abs(float(r["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    with torch.no_grad():
        pexp = OP.perturbation_constraint(p0 + args.lr * torch.from_numpy(g[None]).sign(), clean if norm == "snr" else None, args, spl)
    e_p = rel_err(p.cpu().numpy()[0], pexp.numpy()[0])
    print(f"case {case} {variant}: grad rel {e_g:.2e} flips {flips:.2e} loss rel {e_loss:.2e} p' rel {e_p:.2e}")
    assert e_g < 5e-3 and flips < 5e-3 and e_loss < 2e-4 and e_p < 5e-5, (e_g, flips, e_loss, e_p)


# ---- 4. drawing inside captured graphs; pinned rooms ---------------------------------------------------------------------
def _case(B=2, L=8000, **kw):
    args = cli_to_args("linf", ["--linf_size", "0.01"])
    args.device, args.sr, args.seed = "cuda", 16000, 5
    args.rir_bank, args.rir_count, args.rir_taps = "synthetic", 8, 300
    for k, v in kw.items():
        setattr(args, k, v)
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    return args, m, clean, labels


def test_draws_in_graph_follow_the_device_counters():
    B, L, c0, r0 = 2, 8000, 4, 9
    args, m, clean, labels = _case(B, L, place_shift="random")
    p0 = torch.from_numpy(synth.perturbation(L) * np.float32(1e-3)).cuda().view(1, L)
    st_g, st_e = PgdStepper(m, args, L), PgdStepper(m, args, L)
    p_g, p_e = p0.clone(), p0.clone()
    for st in (st_g, st_e):
        st.set_place_step(c0)
        st.set_rir_step(r0)
    with record_launches() as cap:
        g, _ = st_g.capture(p_g, clean, labels)
    torch.cuda.synchronize()
    seq = ["paa_place_draw", "paa_place_rows", "paa_rir_draw", "paa_rir_apply", "paa_model_fwd_bwd_rows", "paa_rir_apply", "paa_place_reduce",
           "paa_sign_step", "paa_project"]
    assert cap == seq + seq                                      # the warm-up step, then the captured one
    assert int(st_g.placer.counter.item()) == c0 and int(st_g.reverb.counter.item()) == r0      # capture() leaves both counters as it found them
    p_g.copy_(p0)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert st_g.reverb.index.cpu().tolist() == RR.draw(5, r0 + k, 0, B, 0, 8).tolist(), k
        assert st_g.placer.shift.cpu().tolist() == PR.draw(5, c0 + k, 0, B, 0, L)[0].tolist(), k
        assert int(st_g.reverb.counter.item()) == r0 + k + 1 and int(st_g.placer.counter.item()) == c0 + k + 1
        st_e.step(p_e, clean, labels)
        torch.cuda.synchronize()
        assert torch.equal(st_e.reverb.index, st_g.reverb.index) and torch.equal(st_e.placer.shift, st_g.placer.shift)
    assert torch.equal(p_g, p_e) and not torch.equal(p_g, p0)    # three replays = three eager steps


def test_set_rooms_pins_indices():
    B, L = 2, 8000
    args, m, clean, labels = _case(B, L)
    p0 = torch.from_numpy(synth.perturbation(L) * np.float32(1e-3)).cuda().view(1, L)
    st = PgdStepper(m, args, L)
    st.set_rooms([6, 1])
    p = p0.clone()
    for _ in range(2):
        with record_launches() as names:
            st.step(p, clean, labels)
        assert "paa_rir_draw" not in names and "paa_place_draw" not in names and names.count("paa_rir_apply") == 2
    torch.cuda.synchronize()
    assert st.reverb.index.cpu().tolist() == [6, 1] and int(st.reverb.counter.item()) == 0
    want = RR.apply64(rir.bank_of(args), [6, 1], st.placer.rows.cpu().numpy())
    assert np.all(np.abs(st.reverb.rows.cpu().numpy() - want) <= RR.bound(rir.bank_of(args), [6, 1], st.placer.rows.cpu().numpy()))
    assert torch.equal(rir.reverberate(st.placer.rows, rir.bank_of(args), [6, 1]), st.reverb.rows)
    st.set_rooms(None)                                           # back to drawing, from the counter where it stood
    with record_launches() as names:
        st.step(p, clean, labels)
    torch.cuda.synchronize()
    assert "paa_rir_draw" in names and st.reverb.index.cpu().tolist() == RR.draw(5, 0, 0, B, 0, 8).tolist() and int(st.reverb.counter.item()) == 1
    with pytest.raises(ValueError):
        st.set_rooms([0, 1, 2])


# ---- 5. unchanged when off ------------------------------------------------------------------------------------------------
def test_off_is_the_plain_step():
    B, L = 2, 8000
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    outs = []
    for explicit in (False, True):
        args = cli_to_args("snr", ["--snr_db", "40"])
        args.device = "cuda"
        assert not hasattr(args, "rir_bank")
        if explicit:
            args.rir_bank, args.rir_count, args.rir_taps = "none", 4, 100
        st = PgdStepper(m, args, L)
        assert not st.rir_on and not st.place_on and st.Lp == L and st.packed.numel() == L + 8
        for name in ("placer", "reverb", "room", "rir_counter", "wet_rows", "rows", "grad_rows"):
            assert name not in vars(st), name
        with pytest.raises(RuntimeError):
            st.set_rooms([0, 0])
        with pytest.raises(RuntimeError):
            st.set_rir_step(3)
        p = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L)
        labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
        seqs = []
        for _ in range(2):
            with record_launches() as names:
                r = st.step(p, clean, labels)
            seqs.append(names)
        torch.cuda.synchronize()
        assert seqs[0] == seqs[1] == ["paa_model_fwd_bwd", "paa_sign_step", "paa_project"]
        outs.append((p.clone(), r["loss"].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 6. Adam on a short perturbation --------------------------------------------------------------------------------------
def test_adam_on_a_short_perturbation_matches_torch():
    B, L, Lp, lr = 2, 8000, 4096, 2e-4
    args, m, clean, labels = _case(B, L, perturbation_seconds=Lp / 16000, place_shift="random", optimizer_type="adam", lr=lr)
    p0 = torch.from_numpy(synth.perturbation(Lp) * np.float32(1e-3)).cuda().view(1, Lp)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr)
    st = PgdStepper(m, args, L, optimizer=opt)
    assert st.Lp == Lp and st.rir_on
    q = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([q], lr=lr)
    for k in range(3):
        st.step(p.data, clean, labels)
        torch.cuda.synchronize()
        assert p.grad.shape == (1, Lp) and torch.equal(p.grad, -st.grad) and float(st.grad.abs().max()) > 0
        q.grad = p.grad.clone()
        ref.step()
        with torch.no_grad():
            q.clamp_(-float(args.linf_size), float(args.linf_size))
        assert torch.equal(p.detach(), q.detach()), k
    assert torch.equal(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"])
    assert torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])


# ---- 7. two ranks ---------------------------------------------------------------------------------------------------------
def test_two_ranks_equal_one_with_rooms(tmp_path):
    import rir_dist_child as child
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "rir_dist_child.py"),
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
        res.append(json.loads([l for l in so.splitlines() if l.startswith("RIR_CHILD ")][-1][len("RIR_CHILD "):]))
    for d in res:
        assert d["replicas_identical"] and d["graph_equals_eager"] and d["split_graph"] == "_SplitGraph", d
    p_dp = np.load(tmp_path / "rank0.npz")["p_eager"]
    # one rank holding both clips
    L, B = child.L, 2
    args = child.case_args()
    a = A.tiny()
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    p = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L)
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    st = PgdStepper(m, args, L)
    st.set_placement(list(child.SHIFTS))
    st.set_rooms(list(child.ROOMS))
    for _ in range(child.STEPS):
        r = st.step(p, clean, opgd.make_labels(child.TEXTS, args, B))
    torch.cuda.synchronize()
    assert res[0]["loss"] == pytest.approx(float(r["loss"]), rel=1e-5)
    diff = np.abs(p_dp - p.cpu().numpy())
    scale = np.abs(p.cpu().numpy()).max()
    print(f"reverberant DP vs single max diff {diff.max() / scale:.2e}; fraction differing {(diff > 1e-6 * scale).mean():.2e}")
    assert (diff > 1e-5 * scale).mean() < 5e-3          # only where a gradient sign is numerically undecided


# ---- 8. evaluation and the runner -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", [False, True])
def test_evaluate_repeats_its_rooms(placed):
    from paa_amd.core import loss_helpers
    from paa_amd.training_utils import evaluation, parser
    B, L = 2, 8000
    Lp = 4096 if placed else L
    args = parser.create_arg_parser().parse_args(
        ["--arch", "tiny", "--dtype", "fp32", "--norm_type", "linf", "--rir_bank", "synthetic", "--rir_count", "8", "--rir_taps", "300"]
        + (["--place_shift", "random", "--perturbation_seconds", str(Lp / 16000)] if placed else []))
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    x = torch.from_numpy(synth.clean_audio(3 * B, L))
    texts = ["ab cd", "hello", "a b c", "xyz w", "the fox", "dog"]
    loader = [(x[i:i + B], texts[i:i + B]) for i in range(0, 3 * B, B)]
    p = torch.from_numpy(synth.perturbation(Lp) * np.float32(1e-2)).cuda().view(1, Lp)
    s1 = evaluation.evaluate(args, loader, p, m, None, None, perturbed=True)
    s2 = evaluation.evaluate(args, loader, p, m, None, None, perturbed=True)
    assert (s1.ctc, s1.wer) == (s2.ctc, s2.wer)                  # the counters restart: every evaluation hears the same rooms
    bank = rir.bank_of(args)
    ctc, wer = [], []
    for k, (data, tt) in enumerate(loader):
        shifts = PR.draw(int(args.seed), k, 0, B, 1, Lp)[0] if placed else [0] * B
        rooms = RR.draw(int(args.seed), k, 0, B, 1, 8)
        rows = rir.reverberate(place.place_rows(p, L, shifts), bank, rooms)
        r = m.forward(data.cuda(), rows, loss_helpers.make_labels(tt, None, args, B), clamp=False)
        ctc.append(float(r["loss"]))
        e, w = loss_helpers.wer_counts(*loss_helpers.wer_texts(r["logits"], tt, None))
        wer.append(e / max(w, 1))
    assert s1.ctc == pytest.approx(sum(ctc) / 3, rel=1e-6) and s1.wer == pytest.approx(sum(wer) / 3, rel=1e-6, abs=1e-12)
    args.rir_bank = "none"
    dry = evaluation.evaluate(args, loader, p, m, None, None, perturbed=True)
    assert dry.ctc != s1.ctc


def test_runner_writes_and_resumes_with_rooms(tmp_path):
    from paa_amd import run_attack
    from paa_amd.training_utils import parser

    def run(extra):
        args = parser.create_arg_parser().parse_args(
            ["--arch", "tiny", "--audio_seconds", "0.5", "--batch_size", "4", "--steps_per_epoch", "2", "--num_epochs", "2",
             "--logs_dir", str(tmp_path), "--dtype", "fp32", "--silent", "--optimizer_type", "pgd", "--norm_type", "linf",
             "--linf_size", "0.01", "--rir_bank", "synthetic", "--rir_count", "4", "--rir_taps", "200", *extra])
        return run_attack.main(args), args
    rc, args = run([])
    assert rc == 0 and "_rir4x200_" in os.path.basename(args.save_dir) and "_place" not in args.save_dir
    d = json.load(open(os.path.join(args.save_dir, "results.json")))
    assert d["finished_training"] == 1.0 and d["rir_bank"] == "synthetic" and d["rir_count"] == 4 and d["rir_taps"] == 200
    assert "perturbation_length" not in d and "place_shift" not in d           # placement's keys keep their meaning
    p = torch.load(os.path.join(args.save_dir, "perturbation.pt"), weights_only=True)
    assert tuple(p.shape) == (1, 8000) and torch.isfinite(p).all() and float(p.abs().max()) > 0
    rc2, args2 = run(["--num_epochs", "3"])
    assert rc2 == 0 and args2.resume is True and args2.save_dir == args.save_dir
    # a run without the flag keeps the directory and the keys it always had
    args3 = parser.create_arg_parser().parse_args(["--arch", "tiny", "--logs_dir", str(tmp_path), "--norm_type", "linf", "--silent"])
    build.create_logger(args3)
    assert "_rir" not in args3.save_dir
