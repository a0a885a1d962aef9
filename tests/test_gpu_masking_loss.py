"""-m gpu: the masking-threshold loss term against tests/masking_loss_ref.py.  The reference is always fed the
DEVICE's own theta and Pmax (paa_masking_threshold), so masker decisions are shared and only the new arithmetic is under test:
the hinge decisions (d_weight), the adjoint STFT (d_grad), the losses, the ABI's options and errors, then the device steps, the
captured graphs, the data-parallel step and the runners."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import masking_loss_ref as ML
import masking_ref as MR
from gpu_util import rel_err
from oracle import pgd as opgd, wav2vec2 as OW
from oracle.gen_cases import PGD_TEXTS, cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.core.masking import masking_loss, masking_threshold
from paa_amd.model import PaaModel
from paa_amd.training_utils import pgd as P
from paa_amd.training_utils.clip_attack import ClipStepper
from paa_amd.training_utils.pgd import PgdStepper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_OF = lambda L: 1 + L // 256
F = 513
CASES = [(3, 16000, 3e-2), (2, 8737, 3e-2), (2, 10250, 1e-1), (2, 4096, 3e-2), (2, 5000, 3e-2)]
INACTIVE = (3, 16000, 1e-4)


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


def _args(norm="masking", extra=()):
    a = cli_to_args(norm, list(extra))
    a.masking_margin_db = float(getattr(a, "masking_margin_db", 0.0))
    a.device = "cuda"
    return a


def _case(B, L, amp):
    clean = synth.clean_audio(B, L, seed=7 if L in (4096, 5000) else 3)
    d = (np.stack([synth.normal(synth.key_of(f"mask{b}", 3), L) for b in range(B)]) * amp).astype(np.float32)
    return clean, d


def _call(args, d, clean, alpha=None, grad="zeros", want_w=True, want_sum=True):
    """paa_masking_loss on device tensors d (rows, L), clean (B, L).  grad: "zeros", None or a tensor updated in place."""
    rows, L = d.shape
    B = clean.shape[0]
    pr = runtime.get_proj(args, d.device, B, L)
    g = torch.zeros_like(d) if isinstance(grad, str) else grad
    lr = torch.full((B,), -1.0, device=d.device)
    ls = torch.full((1,), -1.0, device=d.device) if want_sum else None
    W = torch.full((rows, T_OF(L), F), -1.0, device=d.device) if want_w else None
    st = _lib.lib().paa_masking_loss(pr.h, runtime.params_of(args), _lib.ptr(d), rows, _lib.ptr(clean), B, L, _lib.ptr(alpha),
                                     _lib.ptr(g), _lib.ptr(lr), _lib.ptr(ls), _lib.ptr(W), _lib.stream_ptr())
    _lib.check(st)
    torch.cuda.synchronize()
    return {"grad": g, "rows": lr, "sum": ls, "W": W}


def _device_threshold(args, clean):
    theta, pmax = masking_threshold(clean, args)
    torch.cuda.synchronize()
    return theta.cpu().numpy().astype(np.float64), pmax.cpu().numpy().astype(np.float64)


def _check_rows(name, d_np, rows_clips, th, pm, out, active_min):
    """rows_clips[r] = the clips that bound perturbation row r.  Decisions, adjoint and losses of one call against the reference."""
    L = d_np.shape[1]
    Wd = out["W"].cpu().numpy().astype(np.float64)
    gd = -out["grad"].cpu().numpy().astype(np.float64)
    lr = out["rows"].cpu().numpy()
    B = len(th)
    ref_rows, slack = np.zeros(B), np.zeros(B)
    for r, clips in enumerate(rows_clips):
        S = MR.stft_tf(d_np[r])
        ths, pms = [th[b] for b in clips], [pm[b] for b in clips]
        Wr, act = ML.weight(S, ths, pms)
        amb = ML.ambiguous(S, ths, pms)
        share = amb.mean()
        ok = ~amb.any(axis=0)
        eW = np.abs(Wd[r] - Wr)[ok].max() / Wr.max() if Wr.max() > 0 else np.abs(Wd[r]).max()
        g_ref = ML.adjoint(Wd[r].copy(), S, L)
        eg = np.abs(gd[r] - g_ref).max() / max(np.abs(g_ref).max(), 1e-300)
        print(f"{name} row {r}: ambiguous {amb.sum()} of {amb.size} ({share:.2e}), active {act.mean():.3f}, "
              f"W err {eW:.2e}, grad err {eg:.2e} of max {np.abs(g_ref).max():.3e}")
        assert share <= 2e-3, (name, r, share)                      # condition on the inputs, from the reference alone
        if active_min:
            assert act.mean() >= active_min, (name, r, act.mean())
        # f32: c_b through exp2 of an exponent of up to ~40 (40 * 2^-24 * ln 2 = 1.7e-6 relative), summed over the clips
        assert eW <= 1e-5, (name, r, eW)
        assert eg <= 5e-5, (name, r, eg)
        lref = ML.loss_rows(S, ths, pms)
        pw = np.abs(S) ** 2
        for i, b in enumerate(clips):
            ref_rows[b] += lref[i]
            slack[b] += ML.scale(pm[b]) * (np.abs(pw - MR.bound(th[b], pm[b]) ** 2) * amb[i]).sum() / pw.size
    for b in range(B):
        print(f"{name} clip {b}: loss {lr[b]:.6e} ref {ref_rows[b]:.6e} rel {abs(lr[b] - ref_rows[b]) / max(ref_rows[b], 1e-300):.2e}")
        assert abs(lr[b] - ref_rows[b]) <= 1e-4 * ref_rows[b] + slack[b], (name, b, lr[b], ref_rows[b], slack[b])
    assert out["sum"].cpu().numpy()[0] == np.float32(lr.astype(np.float64).sum()), name          # f64, clip order


@pytest.mark.parametrize("B,L,amp", CASES)
def test_kernel_vs_reference(B, L, amp):
    """(4) decisions and (5) arithmetic, universal row and per-clip rows."""
    args = _args()
    clean_np, d_np = _case(B, L, amp)
    clean, d = torch.from_numpy(clean_np).cuda(), torch.from_numpy(d_np).cuda()
    th, pm = _device_threshold(args, clean)
    uni = _call(args, d[:1].contiguous(), clean)
    _check_rows(f"uni {B}x{L}", d_np[:1], [list(range(B))], th, pm, uni, 0.10)
    per = _call(args, d, clean)
    _check_rows(f"clip {B}x{L}", d_np, [[b] for b in range(B)], th, pm, per, 0.10)


def test_all_inactive_leaves_gradient_alone():
    B, L, amp = INACTIVE
    args = _args()
    clean_np, d_np = _case(B, L, amp)
    clean, d = torch.from_numpy(clean_np).cuda(), torch.from_numpy(d_np).cuda()
    th, pm = _device_threshold(args, clean)
    for rows in (1, B):
        for r in range(rows):                   # precondition, from the reference alone: nothing active, nothing ambiguous
            clips = list(range(B)) if rows == 1 else [r]
            S = MR.stft_tf(d_np[r])
            ths, pms = [th[b] for b in clips], [pm[b] for b in clips]
            assert not ML.weight(S, ths, pms)[1].any() and not ML.ambiguous(S, ths, pms).any()
        g0 = torch.from_numpy(synth.normal(synth.key_of("g0", 3), rows * L).astype(np.float32).reshape(rows, L)).cuda()
        g0[0, :7] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 3e38])
        g = g0.clone()
        out = _call(args, d[:rows].contiguous(), clean, grad=g)
        assert torch.equal(g.view(torch.int32), g0.view(torch.int32))
        assert (out["rows"] == 0).all() and float(out["sum"]) == 0.0 and (out["W"] == 0).all()


def test_accumulation_alpha_and_options():
    """(6): grad -= alpha * dloss on a non-zero gradient; d_alpha = NULL is alpha = 1; d_grad = NULL leaves the losses."""
    B, L, amp = CASES[0]
    args = _args()
    clean_np, d_np = _case(B, L, amp)
    clean, d = torch.from_numpy(clean_np).cuda(), torch.from_numpy(d_np).cuda()
    for rows in (1, B):
        dd = d[:rows].contiguous()
        base = _call(args, dd, clean)                                                  # zeros, alpha NULL: -grad
        one = _call(args, dd, clean, alpha=torch.ones(1, device="cuda"))
        assert torch.equal(base["grad"], one["grad"]) and torch.equal(base["rows"], one["rows"])
        g0 = torch.from_numpy(synth.normal(synth.key_of("g0", 3), rows * L).astype(np.float32).reshape(rows, L)).cuda()
        al = torch.full((1,), 0.37, device="cuda")
        acc = _call(args, dd, clean, alpha=al, grad=g0.clone())
        nabla = -base["grad"].cpu().numpy().astype(np.float64)
        a32 = float(np.float32(0.37))
        exp = g0.cpu().numpy().astype(np.float64) - a32 * nabla
        err = np.abs(acc["grad"].cpu().numpy().astype(np.float64) - exp)
        # one f32 product and one f32 difference (or their fused form): 2^-23 of the larger operand covers both
        assert (err <= 2.0 ** -23 * np.maximum(np.abs(g0.cpu().numpy()), np.abs(a32 * nabla)) + 1e-38).all(), err.max()
        assert np.abs(a32 * nabla).max() > 1e-3 * np.abs(g0.cpu().numpy()).max()         # the term is visible
        only = _call(args, dd, clean, grad=None, want_w=False)
        assert only["grad"] is None and torch.equal(only["rows"], base["rows"]) and torch.equal(only["sum"], base["sum"])
        nosum = _call(args, dd, clean, want_sum=False)
        assert torch.equal(nosum["rows"], base["rows"]) and torch.equal(nosum["grad"], base["grad"])
        lr, g = masking_loss(dd, clean, args, grad=True)                               # the public function: +grad, alpha = 1
        torch.cuda.synchronize()
        assert torch.equal(lr, base["rows"]) and torch.equal(g, -base["grad"])
        assert masking_loss(dd, clean, args)[1] is None


@pytest.mark.parametrize("B,L,amp", [CASES[0], CASES[1], CASES[4]])
def test_row_identities(B, L, amp):
    """(7): per-clip row b is bit-equal to the one-row, one-clip call; the universal gradient is the sum of the one-clip
    gradients; two identical calls are bit-equal."""
    args = _args()
    clean_np, d_np = _case(B, L, amp)
    clean, d = torch.from_numpy(clean_np).cuda(), torch.from_numpy(d_np).cuda()
    per, per2 = _call(args, d, clean), _call(args, d, clean)
    uni, uni2 = _call(args, d[:1].contiguous(), clean), _call(args, d[:1].contiguous(), clean)
    for k in ("grad", "rows", "sum", "W"):
        assert torch.equal(per[k], per2[k]) and torch.equal(uni[k], uni2[k]), k
    tot = np.zeros(L)
    for b in range(B):
        one = _call(args, d[b:b + 1].contiguous(), clean[b:b + 1].contiguous())
        assert torch.equal(one["grad"][0], per["grad"][b]) and torch.equal(one["W"][0], per["W"][b]), (B, L, b)
        assert torch.equal(one["rows"][0], per["rows"][b])
        o = _call(args, d[:1].contiguous(), clean[b:b + 1].contiguous())
        tot += o["grad"][0].cpu().numpy().astype(np.float64)
        assert o["rows"][0] == uni["rows"][b]
    gu = uni["grad"][0].cpu().numpy().astype(np.float64)
    assert np.abs(gu - tot).max() <= 1e-6 * np.abs(tot).max()


@pytest.mark.parametrize("L", [600, 1300, 2047, 2048, 2304, 2560, 3333])
def test_short_clips(L):
    """Lengths around the launch geometry's edges: T <= 8 is one workgroup holding every frame (both folds may reach the same
    samples), T = 9, 10, 11 are the first shapes with a shifted last workgroup.  Same bounds as (4) and (5)."""
    B, amp = 2, 3e-2
    args = _args()
    clean_np, d_np = _case(B, L, amp)
    clean, d = torch.from_numpy(clean_np).cuda(), torch.from_numpy(d_np).cuda()
    th, pm = _device_threshold(args, clean)
    for rows, clips in ((1, [list(range(B))]), (B, [[b] for b in range(B)])):
        out = _call(args, d[:rows].contiguous(), clean)
        Wd, gd = out["W"].cpu().numpy().astype(np.float64), -out["grad"].cpu().numpy().astype(np.float64)
        for r, cl in enumerate(clips):
            S = MR.stft_tf(d_np[r])
            ths, pms = [th[b] for b in cl], [pm[b] for b in cl]
            Wr, act = ML.weight(S, ths, pms)
            ok = ~ML.ambiguous(S, ths, pms).any(axis=0)
            assert act.any() and np.abs(Wd[r] - Wr)[ok].max() <= 1e-5 * Wr.max(), (L, rows, r)
            g_ref = ML.adjoint(Wd[r].copy(), S, L)
            e = np.abs(gd[r] - g_ref).max() / np.abs(g_ref).max()
            print(f"L={L} T={T_OF(L)} rows={rows} row {r}: grad err {e:.2e}")
            assert e <= 5e-5, (L, rows, r, e)


def test_errors():
    args = _args()
    prm = runtime.params_of(args)
    L = 4096
    pr = runtime.get_proj(args, "cuda", 2, L)
    d = torch.zeros(2, L, device="cuda")
    lib, st = _lib.lib(), _lib.stream_ptr()
    call = lambda h, rows, clean, B: lib.paa_masking_loss(h, prm, _lib.ptr(d), rows, clean, B, L, None, None, _lib.ptr(d[0]),
                                                           None, None, st)
    assert call(pr.h, 1, None, 2) == _lib.PAA_ERR_NEED_CLEAN
    assert call(pr.h, 1, _lib.ptr(d), pr.max_batch + 1) == _lib.PAA_ERR_SIZE
    big = torch.zeros(3, L, device="cuda")
    pr3 = runtime.get_proj(args, "cuda", 3, L)
    assert lib.paa_masking_loss(pr3.h, prm, _lib.ptr(big), 2, _lib.ptr(big), 3, L, None, None, _lib.ptr(big[0]), None, None,
                                st) == _lib.PAA_ERR_ARG
    odd = types.SimpleNamespace(**{**vars(args), "n_fft": 512, "win_length": 512, "hop_length": 128})
    pr2 = runtime.get_proj(odd, "cuda", 2, L)
    assert call(pr2.h, 1, _lib.ptr(d), 2) == _lib.PAA_ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ device steps
TEXTS4 = ["ab cd", "hello", "a b c", "xyz w"]


def _model(variant, B, L):
    a = A.tiny() if variant == "group" else A.tiny("layer", stable=True)
    sdn = A.rule_weights(a)
    return a, sdn, PaaModel(a, sdn, B, L, "fp32")


def _step_args(alpha=None, norm="linf", lr=1e-3):
    args = _args(norm)
    args.linf_size, args.lr = 1e9, lr
    if alpha is not None:
        args.masking_loss_alpha = alpha
    return args


def _step_case(B=2, L=16000, amp=3e-2):
    clean_np, d_np = _case(B, L, amp)
    return torch.from_numpy(clean_np), torch.from_numpy(d_np)


def _ref_terms(variant, clean, d0, rows):
    """Oracle CTC gradient (rows, L) and reference masking-loss gradient / losses for the universal row (rows = 1) or per clip."""
    B, L = clean.shape
    args = _step_args()
    a = A.tiny() if variant == "group" else A.tiny("layer", stable=True)
    sdn = A.rule_weights(a)
    th, pm = _device_threshold(args, clean.cuda())
    sd = OW.to_torch(sdn)
    if rows == 1:
        labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
        g_ctc = opgd.pgd_step(sd, a, args, clean, labels, d0[:1])["grad"].numpy().astype(np.float64)
        clips = [list(range(B))]
    else:
        g_ctc = np.stack([opgd.pgd_step(sd, a, args, clean[b:b + 1], opgd.make_labels([PGD_TEXTS[b]], args, 1),
                                        d0[b:b + 1])["grad"].numpy()[0] for b in range(B)]).astype(np.float64)
        clips = [[b] for b in range(B)]
    g_ml, lsum, slack = [], 0.0, 0.0
    for r, cl in enumerate(clips):
        ths, pms = [th[b] for b in cl], [pm[b] for b in cl]
        g, W, S = ML.grad(d0[r].numpy().astype(np.float64), ths, pms)
        g_ml.append(g)
        lsum += ML.loss_rows(S, ths, pms).sum()
        amb, pw = ML.ambiguous(S, ths, pms), np.abs(S) ** 2
        slack += sum(ML.scale(pm[b]) * (np.abs(pw - MR.bound(th[b], pm[b]) ** 2) * amb[i]).sum() / pw.size for i, b in enumerate(cl))
    return g_ctc, np.stack(g_ml), lsum, slack


@pytest.mark.parametrize("variant", ["group", "layer"])
@pytest.mark.parametrize("rows", ["universal", "per_clip"])
def test_step_vs_oracle(variant, rows):
    """(9): grad = oracle CTC gradient - alpha * reference masking-loss gradient, alpha chosen so that both terms matter;
    p' = p + lr sign(grad) exactly; slot 6 = sum_b l_b; Adam equals torch.optim.Adam fed the device gradient."""
    B, L = 2, 16000
    clean, d0 = _step_case(B, L)
    nrows = 1 if rows == "universal" else B
    g_ctc, g_ml, lsum, slack = _ref_terms(variant, clean, d0, nrows)
    alpha = float(np.abs(g_ctc).max() / np.abs(g_ml).max())
    a32 = float(np.float32(alpha))
    want = g_ctc - a32 * g_ml
    args = _step_args(alpha)
    a, sdn, m = _model(variant, B, L)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    cl = clean.cuda()
    st = PgdStepper(m, args, L) if nrows == 1 else ClipStepper(m, args, L)
    p = d0[:nrows].clone().cuda()
    r = st.step(p, cl, labels)
    torch.cuda.synchronize()
    g = st.grad.cpu().numpy().reshape(nrows, L)
    for b in range(nrows):
        e, sg = rel_err(g[b], want[b]), float((np.sign(g[b]) != np.sign(want[b])).mean())
        plain = rel_err(g[b], g_ctc[b])
        print(f"{variant} {rows} row {b}: alpha {alpha:.3e}, grad rel err {e:.2e}, sign mismatches {sg:.2e}, "
              f"distance to the plain gradient {plain:.2e}")
        assert e < 5e-3 and sg < 5e-3
        assert plain > 0.1                                                      # the loss term is in the gradient
    pexp = d0[:nrows].numpy() + np.float32(args.lr) * np.sign(g).astype(np.float32)
    assert np.array_equal(p.cpu().numpy(), pexp.astype(np.float32))
    slot = float(st.stats[P.ST_MASK_LOSS])
    assert abs(slot - lsum) <= 1e-4 * lsum + slack, (slot, lsum)
    ml = r["masking_loss"]
    if nrows == 1:
        assert ml.dim() == 0 and float(ml) == slot
    else:
        assert ml.shape == (B,) and np.float32(ml.cpu().numpy().astype(np.float64).sum()) == np.float32(slot)
    direct = _call(args, d0[:nrows].clone().cuda(), cl)
    assert float(direct["sum"]) == slot
    # Adam: the same gradient, then torch's update
    pa = torch.nn.Parameter(d0[:nrows].clone().cuda())
    opt = torch.optim.Adam([pa], lr=args.lr)
    sa = PgdStepper(m, args, L, optimizer=opt) if nrows == 1 else ClipStepper(m, args, L, optimizer=opt)
    sa.step(pa.data, cl, labels)
    torch.cuda.synchronize()
    assert torch.equal(sa.grad.reshape(nrows, L), st.grad.reshape(nrows, L))
    pt = torch.nn.Parameter(d0[:nrows].clone().cuda())
    opt_t = torch.optim.Adam([pt], lr=args.lr)
    pt.grad = -sa.grad.reshape(nrows, L).clone()
    opt_t.step()
    torch.cuda.synchronize()
    assert torch.equal(pa.data, pt.data)


def _run_steps(make, p0, clean, labels, steps=3, lr=1e-3):
    st, p = make()
    for _ in range(steps):
        st.step(p.data if isinstance(p, torch.nn.Parameter) else p, clean, labels)
    torch.cuda.synchronize()
    return p.detach().clone(), st.grad.clone(), st.stats.clone()


@pytest.mark.parametrize("opt", ["pgd", "adam"])
@pytest.mark.parametrize("rows", ["universal", "per_clip"])
def test_alpha_zero_is_the_plain_step(opt, rows, monkeypatch):
    """(10): args without the attribute and args with alpha = 0.0 give the same bits, slot 6 stays 0 and paa_masking_loss is
    never called."""
    B, L = 2, 8737
    clean, d0 = _step_case(B, L)
    cl = clean.cuda()
    nrows = 1 if rows == "universal" else B
    a, sdn, m = _model("group", B, L)
    calls = []
    real = _lib.lib().paa_masking_loss
    monkeypatch.setattr(_lib.lib(), "paa_masking_loss", lambda *x: (calls.append(1), real(*x))[1])
    res = {}
    for key, alpha in (("absent", None), ("zero", 0.0)):
        args = _step_args(alpha)
        assert hasattr(args, "masking_loss_alpha") == (alpha is not None)
        labels = opgd.make_labels(PGD_TEXTS[:B], args, B)

        def make():
            p = torch.nn.Parameter(d0[:nrows].clone().cuda()) if opt == "adam" else d0[:nrows].clone().cuda()
            o = torch.optim.Adam([p], lr=args.lr) if opt == "adam" else None
            return (PgdStepper(m, args, L, optimizer=o) if nrows == 1 else ClipStepper(m, args, L, optimizer=o)), p
        res[key] = _run_steps(make, d0, cl, labels)
    for x, y in zip(res["absent"], res["zero"]):
        assert torch.equal(x, y)
    assert float(res["zero"][2][P.ST_MASK_LOSS]) == 0.0 and not calls
    args = _step_args(1e-9)                         # the wrapper does count
    st = PgdStepper(m, args, L)
    r = st.step(d0[:1].clone().cuda(), cl, opgd.make_labels(PGD_TEXTS[:B], args, B))
    torch.cuda.synchronize()
    assert len(calls) == 1 and float(r["masking_loss"]) > 0


@pytest.mark.parametrize("kind", ["pgd", "adam", "clip", "clip_adam"])
def test_replay_equals_eager_and_follows_alpha(kind):
    """(11): eager == captured replay over 3 steps, alpha changed before the third; switching the term off after capture raises."""
    B, L, alpha = 2, 8737, 5e-6
    clean, d0 = _step_case(B, L)
    cl = clean.cuda()
    nrows = B if kind.startswith("clip") else 1
    a, sdn, m = _model("group", B, L)
    args = _step_args(alpha)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    out = {}
    for mode in ("eager", "graph"):
        p = torch.nn.Parameter(d0[:nrows].clone().cuda()) if "adam" in kind else d0[:nrows].clone().cuda()
        o = torch.optim.Adam([p], lr=args.lr) if "adam" in kind else None
        st = PgdStepper(m, args, L, optimizer=o) if nrows == 1 else ClipStepper(m, args, L, optimizer=o)
        pd = p.data if isinstance(p, torch.nn.Parameter) else p
        seen = []
        if mode == "graph":
            g, r = st.capture(pd, cl, labels)
            pd.copy_(d0[:nrows].cuda())
        for i in range(3):
            if i == 2:
                st.set_masking_alpha(4 * alpha)
            if mode == "eager":
                r = st.step(pd, cl, labels)
            else:
                g.replay()
            seen.append(r["masking_loss"].clone())
        torch.cuda.synchronize()
        out[mode] = (pd.clone(), st.grad.clone(), st.stats.clone(), torch.stack([s.reshape(-1) for s in seen]))
        if mode == "graph":
            with pytest.raises(ValueError, match="after capture"):
                st.set_masking_alpha(0.0)
            st.set_masking_alpha(alpha)                 # still allowed
    for x, y in zip(out["eager"], out["graph"]):
        assert torch.equal(x, y)
    # the changed alpha is visible: the same three steps at a constant alpha end elsewhere
    st = PgdStepper(m, args, L) if nrows == 1 else ClipStepper(m, args, L)
    if "adam" not in kind:
        q = d0[:nrows].clone().cuda()
        for i in range(3):
            st.step(q, cl, labels)
        torch.cuda.synchronize()
        assert not torch.equal(q, out["eager"][0])
    # a stepper captured WITHOUT the term cannot gain it
    s0 = PgdStepper(m, _step_args(0.0), L)
    q = d0[:1].clone().cuda()
    s0.capture(q, cl, labels)
    with pytest.raises(ValueError, match="after capture"):
        s0.set_masking_alpha(5e-6)


def test_direction_five_steps_lower_the_loss():
    """(12): with alpha = 100 x the balancing value, five PGD steps take sum_b l_b to <= 0.8 x; with alpha = 0 they do not."""
    B, L = 2, 16000
    clean, d0 = _step_case(B, L)
    cl = clean.cuda()
    g_ctc, g_ml, lsum, _ = _ref_terms("group", clean, d0, 1)
    alpha = 100.0 * float(np.abs(g_ctc).max() / np.abs(g_ml).max())
    a, sdn, m = _model("group", B, L)
    ratio = {}
    for key, al in (("on", alpha), ("off", 0.0)):
        args = _step_args(al, lr=1e-3)
        labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
        st = PgdStepper(m, args, L)
        p = d0[:1].clone().cuda()
        l0 = float(masking_loss(p, cl, args)[0].double().sum())
        for _ in range(5):
            st.step(p, cl, labels)
        ratio[key] = float(masking_loss(p, cl, args)[0].double().sum()) / l0
        assert abs(l0 - lsum) <= 1e-3 * lsum
    print(f"sum_b l_b after five steps / before: alpha {alpha:.3e}: {ratio['on']:.3f}; alpha 0: {ratio['off']:.3f}")
    assert ratio["on"] <= 0.8 and ratio["off"] > 0.95


def test_composite_with_the_masking_norm():
    """(13): --norm_type masking with the loss term: p' is paa_project of p + lr sign(grad), with the stepper's own gradient."""
    B, L = 2, 16000
    clean, d0 = _step_case(B, L)
    cl = clean.cuda()
    a, sdn, m = _model("group", B, L)
    args = _step_args(5e-6, norm="masking")
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    st = PgdStepper(m, args, L)
    p = d0[:1].clone().cuda()
    r = st.step(p, cl, labels)
    plain = PgdStepper(m, _step_args(None, norm="masking"), L)
    pp = d0[:1].clone().cuda()
    plain.step(pp, cl, labels)
    q = d0[:1].clone().cuda()
    lib = _lib.lib()
    _lib.check(lib.paa_sign_step(_lib.ptr(q), _lib.ptr(st.grad), float(args.lr), L, _lib.stream_ptr()))
    _lib.check(lib.paa_project(st.proj.h, runtime.params_of(args), _lib.ptr(q), 1, _lib.ptr(cl), B, L, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(p, q) and float(r["masking_loss"]) > 0
    assert not torch.equal(plain.grad, st.grad)


# ------------------------------------------------------------------------------------------------ data-parallel
DP_ALPHA = 5e-6     # the order of test_step_vs_oracle's balancing alpha (4e-6 .. 1.3e-5, printed there); any alpha > 0 serves here


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, q, sizes, graph):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    a = A.tiny()
    B, L = sizes[rank], 8000
    first = sum(sizes[:rank])
    args = cli_to_args("snr", ["--snr_db", "40"])
    args.device, args.masking_loss_alpha = "cuda", DP_ALPHA
    clean = torch.from_numpy(synth.clean_audio(B, L, first_clip=first)).cuda()
    p = torch.from_numpy(synth.perturbation(L) * np.float32(3e-2)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    st = PgdStepper(m, args, L)
    assert st.world == world and st.collective
    labels = opgd.make_labels(TEXTS4[first:first + B], args, B)
    if graph:
        p0 = p.clone()
        g, r = st.capture(p, clean, labels)
        p.copy_(p0)
        for _ in range(2):
            g.replay()
    else:
        for _ in range(2):
            r = st.step(p, clean, labels)
    torch.cuda.synchronize()
    out = [torch.zeros_like(p) for _ in range(world)]
    dist.all_gather(out, p)
    if rank == 0:
        q.put((p.cpu().numpy(), float(r["loss"]), float(r["masking_loss"]), all(torch.equal(o, out[0]) for o in out)))
    dist.destroy_process_group()


@pytest.mark.parametrize("sizes,graph", [((3, 1), False), ((2, 2), False), ((3, 1), True), ((2, 2), True)])
def test_two_ranks_equal_one(sizes, graph):
    """(14): tests/test_gpu_dist.py::test_two_ranks_equal_one with the loss term on: the term is additive over clips, so it
    rides the SUM all-reduce; slot 6 is reduced like the CTC loss."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, sizes, graph)) for r in range(2)]
    for pr in procs:
        pr.start()
    p_dp, loss_dp, ml_dp, identical = q.get(timeout=300)
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    assert identical
    a = A.tiny()
    B, L = 4, 8000
    args = cli_to_args("snr", ["--snr_db", "40"])
    args.device, args.masking_loss_alpha = "cuda", DP_ALPHA
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    p = torch.from_numpy(synth.perturbation(L) * np.float32(3e-2)).cuda()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    st = PgdStepper(m, args, L)
    for _ in range(2):
        r = st.step(p, clean, opgd.make_labels(TEXTS4, args, B))
    torch.cuda.synchronize()
    assert loss_dp == pytest.approx(float(r["loss"]), rel=1e-5)
    assert ml_dp == pytest.approx(float(r["masking_loss"]), rel=1e-5) and ml_dp > 0
    diff = np.abs(p_dp - p.cpu().numpy())
    scale = np.abs(p.cpu().numpy()).max()
    print(f"sizes {sizes} graph {graph}: DP vs single max diff {diff.max() / scale:.2e}; fraction differing "
          f"{(diff > 1e-5 * scale).mean():.2e}; masking loss {ml_dp:.6e}")
    assert (diff > 1e-5 * scale).mean() < 5e-3
    # the term is in the step: the plain step ends elsewhere
    args0 = cli_to_args("snr", ["--snr_db", "40"])
    args0.device = "cuda"
    s0 = PgdStepper(m, args0, L)
    p2 = torch.from_numpy(synth.perturbation(L) * np.float32(3e-2)).cuda()
    for _ in range(2):
        s0.step(p2, clean, opgd.make_labels(TEXTS4, args0, B))
    torch.cuda.synchronize()
    assert (np.abs(p2.cpu().numpy() - p.cpu().numpy()) > 1e-5 * scale).mean() > 0.05


# ------------------------------------------------------------------------------------------------ runners
def _walk(root, name):
    return [os.path.join(d, name) for d, _, fs in os.walk(root) if name in fs]


@pytest.mark.parametrize("alpha", ["1e-6", None])
def test_run_attack_writes_the_masking_loss(tmp_path, alpha):
    cmd = [sys.executable, "-m", "paa_amd.run_attack", "--arch", "tiny", "--audio_seconds", "0.5", "--batch_size", "2",
           "--steps_per_epoch", "1", "--num_epochs", "1", "--logs_dir", str(tmp_path), "--dtype", "fp32", "--silent",
           "--optimizer_type", "pgd", "--norm_type", "linf"] + (["--masking_loss_alpha", alpha] if alpha else [])
    assert subprocess.run(cmd, cwd=ROOT, timeout=600).returncode == 0
    found = _walk(str(tmp_path), "results.json")
    assert len(found) == 1
    res = json.load(open(found[0]))
    assert res.get("finished_training") == 1.0
    if alpha:
        assert "_ml1e-06_" in found[0]
        assert res["masking_loss_alpha"] == 1e-6 and np.isfinite(res["train_masking_loss"]) and res["train_masking_loss"] >= 0
    else:
        assert "_ml" not in os.path.basename(os.path.dirname(found[0]))
        assert not [k for k in res if "masking" in k]


@pytest.mark.parametrize("alpha", ["1e-6", None])
def test_attack_clips_writes_the_masking_loss(tmp_path, alpha):
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, "-m", "paa_amd.attack_clips", "--arch", "tiny", "--device", "cuda", "--audio_seconds", "0.5",
           "--batch_size", "2", "--steps_per_epoch", "1", "--small_data", "--silent", "--norm_type", "linf",
           "--pgd_steps", "3", "--optimizer_type", "pgd", "--num_items_to_inspect", "2", "--logs_dir", logs] \
        + (["--masking_loss_alpha", alpha] if alpha else [])
    assert subprocess.run(cmd, cwd=ROOT, timeout=600).returncode == 0
    found = _walk(logs, "clip_results.json")
    assert len(found) == 1
    res = json.load(open(found[0]))
    assert res["clips"]
    if alpha:
        assert "_ml1e-06_" in found[0]
        assert all(np.isfinite(c["final_masking_loss"]) and c["final_masking_loss"] >= 0 for c in res["clips"])
    else:
        assert not any("final_masking_loss" in c for c in res["clips"]) and "_ml" not in found[0].replace(str(tmp_path), "")
