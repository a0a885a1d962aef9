"""-m gpu: random placement of the universal perturbation — the three kernels against tests/place_ref.py, the
placed step against the oracle, the draw inside captured graphs, Adam on a short perturbation, two ranks, evaluation and the runner.

Bounds.  paa_place_rows does one f32 multiply per element: bit-equal to numpy float32.  paa_place_reduce adds exact f64 terms in
f64 and rounds once: |dev - ref64| <= 2^-24 |ref64| + n 2^-52 sum|terms| + 2^-149 per output.  The step bounds are those of
test_gpu_clip_attack._clip_step_vs_oracle.  Every kernel output lives between two guard blocks that must survive."""
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
from gpu_util import rel_err
from oracle import pgd as opgd, projections as OP, wav2vec2 as OW
from oracle.gen_cases import PGD_TEXTS, cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.model import PaaModel
from paa_amd.training_utils import build, place
from paa_amd.training_utils.pgd import PgdStepper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -0x21524111                  # 0xDEADBEEF
CASES = [(3, 5000, 5000), (3, 5000, 1536), (2, 8737, 4096), (2, 10250, 10250), (3, 5000, 7000), (2, 600, 1), (2, 600, 3)]
GAINS = [0.5, 1.0, 1.7]


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    """max_phon contours are loaded into the process-wide projection contexts: drop them for the modules that follow."""
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


class Guarded:
    """A 4-byte device tensor between two guard blocks of a sentinel pattern; the tensor itself starts as the sentinel too."""

    def __init__(self, shape, dtype=torch.float32):
        shape = tuple(int(s) for s in shape)
        self.n, self.g = int(np.prod(shape)), 256
        self.full = torch.full((self.n + 2 * self.g,), SENT, dtype=torch.int32, device="cuda")
        self.t = self.full[self.g:self.g + self.n].view(dtype).view(shape)

    @property
    def ptr(self):
        return _lib.ptr(self.t)

    def check(self):
        assert bool((self.full[:self.g] == SENT).all()) and bool((self.full[self.g + self.n:] == SENT).all()), "guard overwritten"

    def untouched(self):
        return bool((self.full[self.g:self.g + self.n] == SENT).all())


def _shift_sets(B, Lp):
    """0, 1, 255, Lp - 1 and the out-of-range Lp + 5 and -1, B per call"""
    vals = [0, 1, 255, Lp - 1, Lp + 5, -1]
    return [vals[i:i + B] for i in range(0, len(vals), B)]


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def _f32(x):
    return torch.tensor(list(x), dtype=torch.float32, device="cuda")


def _rows(p, Lp, shift, gain, B, L):
    out = Guarded((B, L))
    _lib.check(_lib.lib().paa_place_rows(_lib.ptr(p), Lp, _lib.ptr(shift), _lib.ptr(gain), out.ptr, B, L, _lib.stream_ptr()))
    torch.cuda.synchronize()
    out.check()
    return out.t


def _reduce(G, shift, gain, B, L, Lp):
    out = Guarded((Lp,))
    _lib.check(_lib.lib().paa_place_reduce(_lib.ptr(G), _lib.ptr(shift), _lib.ptr(gain), out.ptr, B, L, Lp, _lib.stream_ptr()))
    torch.cuda.synchronize()
    out.check()
    return out.t


# ---- 1. paa_place_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,Lp", CASES)
def test_place_rows_bit_equal(B, L, Lp):
    p_np = synth.normal(synth.key_of(f"place{Lp}", 5), Lp).astype(np.float32)
    p = torch.from_numpy(p_np).cuda()
    for shifts in _shift_sets(B, Lp):
        for gains in (None, GAINS[:B]):
            got = _rows(p, Lp, _i32(shifts), None if gains is None else _f32(gains), B, L).cpu().numpy()
            ref = PR.place(p_np, L, shifts, gains)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (B, L, Lp, shifts, gains)
    if Lp == L:          # shift 0 and no gain: the broadcast the plain step uses
        got = _rows(p, Lp, _i32([0] * B), None, B, L)
        assert torch.equal(got, p.view(1, L).expand(B, L))


# ---- 2. paa_place_reduce -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,Lp", CASES)
def test_place_reduce(B, L, Lp):
    p64 = synth.normal(synth.key_of(f"place{Lp}", 5), Lp).astype(np.float32).astype(np.float64)
    G_np = np.stack([synth.normal(synth.key_of(f"G{b}_{L}", 5), L) for b in range(B)]).astype(np.float32)
    G = torch.from_numpy(G_np).cuda()
    g32 = np.asarray(GAINS[:B], dtype=np.float32)
    for shifts in _shift_sets(B, Lp):
        sh, ga = _i32(shifts), _f32(GAINS[:B])
        a = _reduce(G, sh, ga, B, L, Lp)
        b = _reduce(G, sh, ga, B, L, Lp)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                 # two calls: the same bits
        dev = a.cpu().numpy()
        ref, mag, cnt = PR.reduce64(G_np, shifts, g32, Lp)
        bound = 2.0 ** -24 * np.abs(ref) + cnt * 2.0 ** -52 * mag + 2.0 ** -149
        err = np.abs(dev.astype(np.float64) - ref)
        print(f"B={B} L={L} Lp={Lp} shifts={shifts}: max err / bound {float((err / bound).max()):.3f}, "
              f"outputs without a term {int((cnt == 0).sum())}")
        assert np.all(err <= bound), (shifts, float((err / bound).max()))
        assert np.all(dev.view(np.uint32)[cnt == 0] == 0)                            # untouched outputs: exactly +0.0f
        if Lp > L:
            assert (cnt == 0).any()
        # <rows(p), G> = <p, reduce(G)> in float64
        lhs = math.fsum((PR.place(p64, L, shifts, g32.astype(np.float64), dtype=np.float64) * G_np.astype(np.float64)).ravel())
        rhs = math.fsum(p64 * dev.astype(np.float64))
        assert abs(lhs - rhs) <= math.fsum(np.abs(p64) * bound), (shifts, lhs, rhs)


# ---- 3. paa_place_draw ---------------------------------------------------------------------------------------------------
def _draw(seed, counter, stream_id, clip_base, B, Lp, shift_on, G, shift, gain):
    return _lib.lib().paa_place_draw(seed, _lib.ptr(counter), stream_id, clip_base, B, Lp, shift_on, G, shift.ptr, gain.ptr,
                                     _lib.stream_ptr())


@pytest.mark.parametrize("Lp", [1000, 16000])
def test_place_draw(Lp):
    for B in (5, 1, 257):          # 257: one past the block, the draw's clip loop takes a second pass
        _place_draw(Lp, B)


def _place_draw(Lp, B):
    base, seed = 7, 5
    counter = Guarded((1,), torch.int32)
    for shift_on, G in ((1, 0.0), (1, 6.0), (0, 6.0)):
        counter.t.zero_()
        for step in range(3):
            shift, gain = Guarded((B,), torch.int32), Guarded((B,))
            _lib.check(_draw(seed, counter.t, 0, base, B, Lp, shift_on, G, shift, gain))
            torch.cuda.synchronize()
            for g in (shift, gain, counter):
                g.check()
            s_ref, a_ref = PR.draw(seed, step, base, B, 0, Lp, bool(shift_on), G)
            assert shift.t.cpu().tolist() == s_ref.tolist(), (step, shift_on, G)
            got = gain.t.cpu().numpy()
            if G == 0.0:
                assert np.all(got == np.float32(1.0))
            else:
                rel = np.abs(got.astype(np.float64) - a_ref) / a_ref
                print(f"Lp={Lp} step={step}: gain max rel err {rel.max():.2e}")
                assert np.all(rel <= 1e-6) and got.min() >= 10 ** (-6 / 20) * (1 - 1e-6) and got.max() <= 10 ** (6 / 20) * (1 + 1e-6)
        assert int(counter.t.item()) == 3
    # the evaluation stream and another seed draw other shifts
    shift, gain = Guarded((B,), torch.int32), Guarded((B,))
    counter.t.zero_()
    _lib.check(_draw(seed + (1 << 32), counter.t, 1, base, B, Lp, 1, 0.0, shift, gain))
    torch.cuda.synchronize()
    assert shift.t.cpu().tolist() == PR.draw(seed + (1 << 32), 0, base, B, 1, Lp)[0].tolist()
    assert shift.t.cpu().tolist() != PR.draw(seed, 0, base, B, 0, Lp)[0].tolist()


def test_place_refusals_leave_outputs_alone():
    L_ = _lib.lib()
    B, L, Lp = 2, 600, 100
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    shift, gain, rows, grad = Guarded((B,), torch.int32), Guarded((B,)), Guarded((B, L)), Guarded((Lp,))
    p, G = torch.zeros(Lp, device="cuda"), torch.zeros(B, L, device="cuda")
    sh, ga = _i32([0, 1]), _f32([1.0, 1.0])
    st = _lib.stream_ptr()
    ARG = _lib.PAA_ERR_ARG
    for g in (-0.5, 20.5, float("nan")):
        assert _draw(5, counter, 0, 0, B, Lp, 1, g, shift, gain) == ARG
    assert _draw(5, counter, 0, 0, 0, Lp, 1, 0.0, shift, gain) == ARG
    assert _draw(5, counter, 0, 0, B, 0, 1, 0.0, shift, gain) == ARG
    assert L_.paa_place_draw(5, None, 0, 0, B, Lp, 1, 0.0, shift.ptr, gain.ptr, st) == ARG
    for B_, L__, Lp_ in ((0, L, Lp), (B, 0, Lp), (B, L, 0)):
        assert L_.paa_place_rows(_lib.ptr(p), Lp_, _lib.ptr(sh), None, rows.ptr, B_, L__, st) == ARG
        assert L_.paa_place_reduce(_lib.ptr(G), _lib.ptr(sh), _lib.ptr(ga), grad.ptr, B_, L__, Lp_, st) == ARG
    assert L_.paa_place_rows(None, Lp, _lib.ptr(sh), None, rows.ptr, B, L, st) == ARG
    assert L_.paa_place_reduce(_lib.ptr(G), _lib.ptr(sh), None, grad.ptr, B, L, Lp, st) == ARG
    with pytest.raises(_lib.PaaError):
        _lib.check(L_.paa_place_reduce(_lib.ptr(G), None, _lib.ptr(ga), grad.ptr, B, L, Lp, st))
    torch.cuda.synchronize()
    assert int(counter.item()) == 0
    for g in (shift, gain, rows, grad):
        g.check()
        assert g.untouched()


# ---- 4. the placed step against the oracle -------------------------------------------------------------------------------
STEP_CASES = {"a": ("linf", [], 16000, (0, 0), None),
              "b": ("snr", ["--snr_db", "40"], 16000, (5555, 143), None),
              "c": ("max_phon", [], 4096, (12, 4095), (0.7, 1.3))}


@pytest.mark.parametrize("variant", ["group", "layer"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_placed_step_vs_oracle(case, variant):
    norm, extra, Lp, shifts, gains = STEP_CASES[case]
    a = A.tiny("group", False) if variant == "group" else A.tiny("layer", True)
    B, L = 2, 16000
    args = cli_to_args(norm, extra)
    args.device = "cuda"
    args.perturbation_seconds = Lp / 16000
    sdn = A.rule_weights(a)
    sd = OW.to_torch(sdn)
    clean = torch.from_numpy(synth.clean_audio(B, L))
    p0 = torch.from_numpy(synth.perturbation(Lp) * np.float32(1e-3)).view(1, Lp)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    spl = OP.spl_thresh_tensor(args)
    m = PaaModel(a, sdn, B, L, "fp32")
    st = PgdStepper(m, args, L, None, build.init_phon_threshold_tensor(args))
    assert st.place_on and st.Lp == Lp and st.packed.numel() == Lp + 8 and st.placer.rows.shape == (B, L) and st.placer.grad_rows.shape == (B, L)
    st.set_placement(shifts, gains)
    p = p0.cuda()
    r = st.step(p, clean.cuda(), labels)
    torch.cuda.synchronize()
    g = st.grad.cpu().numpy()[0]
    g32 = None if gains is None else np.asarray(gains, dtype=np.float32)
    rows0 = torch.from_numpy(PR.place(p0.numpy()[0], L, shifts, g32))
    assert torch.equal(st.placer.rows.cpu(), rows0)
    ref = opgd.pgd_step(sd, a, args, clean, labels, rows0, spl)
    gref = PR.reduce64(ref["grad"].numpy(), shifts, g32, Lp)[0]
    e_g = rel_err(g, gref)
    flips = float((np.sign(g) != np.sign(gref)).mean())
    e_loss = abs(float(r["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    with torch.no_grad():
        pexp = OP.perturbation_constraint(p0 + args.lr * torch.from_numpy(g[None]).sign(), clean if norm == "snr" else None, args, spl)
    e_p = rel_err(p.cpu().numpy()[0], pexp.numpy()[0])
    print(f"case {case} {variant}: grad rel {e_g:.2e} flips {flips:.2e} loss rel {e_loss:.2e} p' rel {e_p:.2e}")
    assert e_g < 5e-3 and flips < 5e-3 and e_loss < 2e-4 and e_p < 5e-5, (e_g, flips, e_loss, e_p)
    if case == "a":          # the placement-off stepper on the same inputs
        off = PgdStepper(m, cli_to_args(norm, extra), L)
        assert not off.place_on
        logits_on, loss_on, g_on = r["logits"].clone(), r["loss"].clone(), st.grad.clone()
        q = p0.cuda()
        ro = off.step(q, clean.cuda(), labels)
        torch.cuda.synchronize()
        assert torch.equal(ro["logits"], logits_on) and torch.equal(ro["loss"], loss_on)
        e_off = rel_err(g_on.cpu().numpy(), off.grad.cpu().numpy())
        print(f"case a {variant}: gradient vs the placement-off step rel {e_off:.2e}; p' equal {torch.equal(p, q)}")
        assert e_off < 1e-6


# ---- 5. drawing inside captured graphs; Adam on a short perturbation -----------------------------------------------------
def _draw_case(B=2, L=8000, **kw):
    args = cli_to_args("linf", ["--linf_size", "0.01"])
    args.device, args.place_shift, args.seed = "cuda", "random", 5
    for k, v in kw.items():
        setattr(args, k, v)
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    return args, m, clean, labels


def test_draw_in_graph_follows_the_device_counter():
    B, L, c0 = 2, 8000, 4
    args, m, clean, labels = _draw_case(B, L, place_gain_db=6.0)
    p0 = torch.from_numpy(synth.perturbation(L) * np.float32(1e-3)).cuda().view(1, L)
    st_g, st_e = PgdStepper(m, args, L), PgdStepper(m, args, L)
    p_g, p_e = p0.clone(), p0.clone()
    st_g.set_place_step(c0)
    st_e.set_place_step(c0)
    g, _ = st_g.capture(p_g, clean, labels)
    torch.cuda.synchronize()
    assert int(st_g.placer.counter.item()) == c0                       # the warm-up step's draw is taken back
    p_g.copy_(p0)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        s_ref, a_ref = PR.draw(5, c0 + k, 0, B, 0, L, True, 6.0)
        assert st_g.placer.shift.cpu().tolist() == s_ref.tolist(), k
        assert np.all(np.abs(st_g.placer.gain.cpu().numpy() - a_ref) <= 1e-6 * a_ref)
        assert int(st_g.placer.counter.item()) == c0 + k + 1
        st_e.step(p_e, clean, labels)
        torch.cuda.synchronize()
        assert torch.equal(st_e.placer.shift, st_g.placer.shift) and torch.equal(st_e.placer.gain, st_g.placer.gain)
    assert torch.equal(p_g, p_e)                                 # three replays = three eager steps
    assert not torch.equal(p_g, p0)


def test_adam_on_a_short_perturbation_matches_torch():
    B, L, Lp, lr = 2, 8000, 4096, 2e-4
    args, m, clean, labels = _draw_case(B, L, perturbation_seconds=Lp / 16000, optimizer_type="adam", lr=lr)
    p0 = torch.from_numpy(synth.perturbation(Lp) * np.float32(1e-3)).cuda().view(1, Lp)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr)
    st = PgdStepper(m, args, L, optimizer=opt)
    assert st.Lp == Lp
    q = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([q], lr=lr)
    for k in range(3):
        st.step(p.data, clean, labels)
        torch.cuda.synchronize()
        assert p.grad.shape == (1, Lp) and torch.equal(p.grad, -st.grad)
        q.grad = p.grad.clone()
        ref.step()
        with torch.no_grad():
            q.clamp_(-float(args.linf_size), float(args.linf_size))
        assert torch.equal(p.detach(), q.detach()), k
    assert torch.equal(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"])
    assert torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])


# ---- 6. unchanged when off ------------------------------------------------------------------------------------------------
def test_off_is_the_plain_step():
    B, L = 2, 8000
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    outs = []
    for explicit in (False, True):
        args = cli_to_args("snr", ["--snr_db", "40"])
        args.device = "cuda"
        assert not hasattr(args, "place_shift")
        if explicit:
            args.perturbation_seconds, args.place_shift, args.place_gain_db = None, "none", 0.0
        st = PgdStepper(m, args, L)
        assert not st.place_on and st.Lp == L and st.packed.numel() == L + 8
        for name in ("placer", "shift", "gain", "counter", "rows", "grad_rows"):
            assert name not in vars(st), name
        with pytest.raises(RuntimeError):
            st.set_placement([0, 0])
        p = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L)
        labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
        for _ in range(2):
            r = st.step(p, clean, labels)
        torch.cuda.synchronize()
        outs.append((p.clone(), r["loss"].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 7. two ranks ---------------------------------------------------------------------------------------------------------
def test_two_ranks_equal_one_with_placement(tmp_path):
    import place_dist_child as child
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "place_dist_child.py"),
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
        res.append(json.loads([l for l in so.splitlines() if l.startswith("PLACE_CHILD ")][-1][len("PLACE_CHILD "):]))
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
    for _ in range(child.STEPS):
        r = st.step(p, clean, opgd.make_labels(child.TEXTS, args, B))
    torch.cuda.synchronize()
    assert res[0]["loss"] == pytest.approx(float(r["loss"]), rel=1e-5)
    diff = np.abs(p_dp - p.cpu().numpy())
    scale = np.abs(p.cpu().numpy()).max()
    print(f"placed DP vs single max diff {diff.max() / scale:.2e}; fraction differing {(diff > 1e-6 * scale).mean():.2e}")
    assert (diff > 1e-5 * scale).mean() < 5e-3          # only where a gradient sign is numerically undecided


# ---- 8. evaluation and the runner -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_wer", [False, True])
def test_evaluate_with_placement(device_wer):
    from paa_amd.core import loss_helpers
    from paa_amd.training_utils import evaluation, parser
    B, L, Lp = 2, 8000, 4096
    args = parser.create_arg_parser().parse_args(["--arch", "tiny", "--dtype", "fp32", "--norm_type", "linf", "--place_shift", "random",
                                                  "--perturbation_seconds", str(Lp / 16000)] + (["--device_wer"] if device_wer else []))
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    x = torch.from_numpy(synth.clean_audio(3 * B, L))
    texts = ["ab cd", "hello", "a b c", "xyz w", "the fox", "dog"]
    loader = [(x[i:i + B], texts[i:i + B]) for i in range(0, 3 * B, B)]
    p = torch.from_numpy(synth.perturbation(Lp) * np.float32(1e-2)).cuda().view(1, Lp)
    s1 = evaluation.evaluate(args, loader, p, m, None, None, perturbed=True)
    s2 = evaluation.evaluate(args, loader, p, m, None, None, perturbed=True)
    assert (s1.ctc, s1.wer) == (s2.ctc, s2.wer)                  # the counter restarts: every evaluation sees the same placements
    ctc, wer = [], []
    for k, (data, tt) in enumerate(loader):
        shifts = PR.draw(int(args.seed), k, 0, B, 1, Lp)[0]
        rows = place.place_rows(p, L, shifts)
        assert torch.equal(rows.cpu(), torch.from_numpy(PR.place(p.cpu().numpy()[0], L, shifts)))
        data = data.cuda()
        r = m.forward(data, rows, loss_helpers.make_labels(tt, None, args, B), clamp=False)
        ctc.append(float(r["loss"]))
        e, w = loss_helpers.wer_counts(*loss_helpers.wer_texts(r["logits"], tt, None))
        wer.append(e / max(w, 1))
    assert s1.ctc == pytest.approx(sum(ctc) / 3, rel=1e-6) and s1.wer == pytest.approx(sum(wer) / 3, rel=1e-6, abs=1e-12)
    clean = evaluation.evaluate(args, loader, 0, m, None, None, perturbed=False)
    assert clean.ctc != s1.ctc


def test_runner_writes_and_resumes_a_short_perturbation(tmp_path):
    import wave
    from paa_amd import run_attack
    from paa_amd.training_utils import parser

    def run(extra):
        args = parser.create_arg_parser().parse_args(
            ["--arch", "tiny", "--audio_seconds", "0.5", "--batch_size", "4", "--steps_per_epoch", "2", "--num_epochs", "2",
             "--logs_dir", str(tmp_path), "--dtype", "fp32", "--silent", "--optimizer_type", "pgd", "--norm_type", "linf",
             "--linf_size", "0.01", "--perturbation_seconds", "0.25", "--place_shift", "random", "--place_gain_db", "3", *extra])
        return run_attack.main(args), args
    rc, args = run([])
    assert rc == 0 and "_place4000sg3_" in os.path.basename(args.save_dir)
    d = json.load(open(os.path.join(args.save_dir, "results.json")))
    assert d["finished_training"] == 1.0 and d["perturbation_length"] == 4000 and d["place_shift"] == "random" and d["place_gain_db"] == 3.0
    p = torch.load(os.path.join(args.save_dir, "perturbation.pt"), weights_only=True)
    assert tuple(p.shape) == (1, 4000) and torch.isfinite(p).all() and float(p.abs().max()) > 0
    with wave.open(os.path.join(args.save_dir, "perturbation.wav"), "rb") as w:
        assert w.getnframes() == 4000
    rc2, args2 = run(["--num_epochs", "3"])
    assert rc2 == 0 and args2.resume is True and args2.save_dir == args.save_dir
    # a run without the flags keeps the directory and the keys it always had
    args3 = parser.create_arg_parser().parse_args(["--arch", "tiny", "--logs_dir", str(tmp_path), "--norm_type", "linf", "--silent"])
    build.create_logger(args3)
    assert "_place" not in args3.save_dir
