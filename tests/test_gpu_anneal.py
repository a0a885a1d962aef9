"""-m gpu: the per-clip adaptive masking-loss weight.  paa_masking_loss_rows row by row against scalar
paa_masking_loss calls, bit for bit; paa_clip_anneal bit for bit against tests/anneal_ref.py; the schedule's ClipStepper (eager, then
captured and replayed) against a loop that runs the same entries but decides on the host; the stepper with the schedule off; the
entry point with --alpha_search qin, alone and as stage 2 of the two-stage run."""
import json
import os

import numpy as np
import pytest
import torch

import anneal_ref as AR
import search_ref as SR
from gpu_util import record_launches
from oracle import pgd as opgd
from oracle.gen_cases import cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.core import loss_helpers
from paa_amd.core.masking import masking_loss
from paa_amd.model import PaaModel
from paa_amd.training_utils import pgd
from paa_amd.training_utils.clip_attack import AnnealConfig, ClipStepper
from test_gpu_search import OTHER, ROW_TOL, Guarded, _free_port, _host_counts, _hyp, _results, _run_entry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


def _args(alpha0=None):
    a = cli_to_args("linf", ["--linf_size", "0.05", "--lr", "0.01"])
    a.masking_margin_db = float(getattr(a, "masking_margin_db", 0.0))
    a.device = "cuda"
    if alpha0 is not None:
        a.masking_loss_alpha = alpha0
    return a


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- 1. per-row alpha against scalar calls --------------------------------------------------------------------------------------
ALPHAS = (3e-6, 1.1e-5, 1.7e-5)


def _mloss(pr, prm, d, clean, alpha, alpha_rows, grad, entry="rows"):
    """One call of either entry on device tensors; returns (status, loss_rows, loss_sum) with grad updated in place."""
    rows, L = d.shape
    B = clean.shape[0]
    lr, ls = torch.full((B,), -1.0, device="cuda"), torch.full((1,), -1.0, device="cuda")
    lib = _lib.lib()
    if entry == "rows":
        st = lib.paa_masking_loss_rows(pr.h, prm, _lib.ptr(d), rows, _lib.ptr(clean), B, L, _lib.ptr(alpha), alpha_rows, _lib.ptr(grad),
                                       _lib.ptr(lr), _lib.ptr(ls), None, _lib.stream_ptr())
    else:
        st = lib.paa_masking_loss(pr.h, prm, _lib.ptr(d), rows, _lib.ptr(clean), B, L, _lib.ptr(alpha), _lib.ptr(grad), _lib.ptr(lr),
                                  _lib.ptr(ls), None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return st, lr, ls


@pytest.mark.parametrize("B,L", [(3, 16000), (2, 8737), (2, 1500)])
def test_rows_alpha_vs_scalar_calls(B, L):
    """(2, 8737): T = 35, the shifted last workgroup; (2, 1500): T = 6, the one-workgroup shape."""
    args = _args()
    prm = runtime.params_of(args, "masking")
    pr = runtime.get_proj(args, "cuda", B, L)
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=3)).cuda()
    d = torch.from_numpy((np.stack([synth.normal(synth.key_of(f"mask{b}", 3), L) for b in range(B)]) * 1e-2).astype(np.float32)).cuda()
    g0 = torch.from_numpy(np.random.default_rng(L).standard_normal((B, L)).astype(np.float32)).cuda()      # a prefilled gradient
    alphas = torch.tensor(ALPHAS[:B], dtype=torch.float32, device="cuda")
    g = g0.clone()
    st, lr, ls = _mloss(pr, prm, d, clean, alphas, B, g)
    assert st == _lib.PAA_OK
    print(f"({B}, {L}): l_b {lr.tolist()}  sum {float(ls)}")
    assert bool((lr > 0).all()), "the term is in play for every clip"
    assert not torch.equal(g, g0)
    # row b == the one-row, one-clip scalar call with alpha_b on the same prefilled row
    for b in range(B):
        gb = g0[b:b + 1].clone()
        st1, lr1, _ = _mloss(pr, prm, d[b:b + 1].contiguous(), clean[b:b + 1].contiguous(), alphas[b:b + 1].clone(), 1, gb, "scalar")
        assert st1 == _lib.PAA_OK
        assert np.array_equal(_bits(g[b]), _bits(gb[0])), (B, L, b, "gradient row")
        assert np.array_equal(_bits(lr[b:b + 1]), _bits(lr1)), (B, L, b, "loss row")
        assert not torch.equal(gb, g0[b:b + 1])
    # all alpha_b equal == the scalar B-row call; loss_sum as before
    one = alphas[1:2].clone()
    ga, gs = g0.clone(), g0.clone()
    st_a, lr_a, ls_a = _mloss(pr, prm, d, clean, one.expand(B).contiguous(), B, ga)
    st_s, lr_s, ls_s = _mloss(pr, prm, d, clean, one, 1, gs, "scalar")
    assert st_a == st_s == _lib.PAA_OK
    assert np.array_equal(_bits(ga), _bits(gs)) and np.array_equal(_bits(lr_a), _bits(lr_s)) and np.array_equal(_bits(ls_a), _bits(ls_s))
    assert np.array_equal(_bits(ls), _bits(ls_s)) and np.array_equal(_bits(lr), _bits(lr_s))       # the losses carry no alpha
    # alpha_rows = 1 through the new entry == paa_masking_loss: a device scalar, NULL (1.0), and the one row against all clips
    for al in (one, None):
        gn, go = g0.clone(), g0.clone()
        _, lr_n, ls_n = _mloss(pr, prm, d, clean, al, 1, gn)
        _, lr_o, ls_o = _mloss(pr, prm, d, clean, al, 1, go, "scalar")
        assert np.array_equal(_bits(gn), _bits(go)) and np.array_equal(_bits(lr_n), _bits(lr_o)) and np.array_equal(_bits(ls_n), _bits(ls_o))
    gn, go = g0[:1].clone(), g0[:1].clone()
    _, lr_n, _ = _mloss(pr, prm, d[:1].contiguous(), clean, one, 1, gn)
    _, lr_o, _ = _mloss(pr, prm, d[:1].contiguous(), clean, one, 1, go, "scalar")
    assert np.array_equal(_bits(gn), _bits(go)) and np.array_equal(_bits(lr_n), _bits(lr_o))
    # the Python entry: gradient row b is alpha_b grad l_b (positive, on a zero gradient), host and device alphas alike
    rows_h, gh = masking_loss(d, clean, args, grad=True, alpha=list(ALPHAS[:B]))
    rows_d, gd = masking_loss(d, clean, args, grad=True, alpha=alphas)
    z = torch.zeros_like(d)
    _mloss(pr, prm, d, clean, alphas, B, z)
    assert torch.equal(gh, gd) and torch.equal(gh, -z) and torch.equal(rows_h, lr) and torch.equal(rows_d, lr)


def test_rows_alpha_argument_contract():
    B, L = 2, 1500
    args = _args()
    prm = runtime.params_of(args, "masking")
    pr = runtime.get_proj(args, "cuda", B, L)
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=3)).cuda()
    d = torch.randn(B, L, device="cuda") * 1e-2
    al = torch.full((B,), 1e-5, device="cuda")
    g = Guarded((B, L))
    g.t.view(torch.int32).fill_(7)
    bad = [dict(alpha=al, alpha_rows=0), dict(alpha=al, alpha_rows=3), dict(alpha=al, alpha_rows=-1),
           dict(alpha=None, alpha_rows=B),                              # per-row weights need the array
           dict(alpha=al, alpha_rows=B, rows=1)]                        # ... and one perturbation row per clip
    with record_launches() as names:
        for kw in bad:
            dd = d[:kw.get("rows", B)].contiguous()
            st, _, _ = _mloss(pr, prm, dd, clean, kw["alpha"], kw["alpha_rows"], g.t[:dd.shape[0]])
            assert st == _lib.PAA_ERR_ARG, kw
            assert b"paa_masking_loss_rows" in _lib.lib().paa_last_error()
    assert set(names) == {"paa_masking_loss_rows", "paa_last_error"}
    assert bool((g.t.view(torch.int32) == 7).all())
    g.check()
    with pytest.raises(ValueError, match="finite and >= 0"):
        masking_loss(d, clean, args, alpha=[1e-5, -1.0])
    with pytest.raises(ValueError, match="one perturbation row per clip"):
        masking_loss(d[:1], clean, args, alpha=[1e-5, 1e-5])


# ---- 2. paa_clip_anneal alone -----------------------------------------------------------------------------------------------------
def _anneal_call(delta, counts, loss, targeted, milli, up_every, down_every, up, down, lo, hi, alpha, best, bloss, balpha, bstep, step):
    B, L = delta.shape
    return _lib.lib().paa_clip_anneal(_lib.ptr(delta), B, L, _lib.ptr(counts), _lib.ptr(loss), int(targeted), int(milli), int(up_every),
                                      int(down_every), float(up), float(down), float(lo), float(hi), _lib.ptr(alpha), _lib.ptr(best),
                                      _lib.ptr(bloss), _lib.ptr(balpha), _lib.ptr(bstep), _lib.ptr(step), _lib.stream_ptr())


@pytest.mark.parametrize("targeted", [False, True])
@pytest.mark.parametrize("L,offset", [(4096, 0), (4099, 0), (4096, 1)])
def test_clip_anneal_vs_reference(L, offset, targeted):
    """B = 7 rows over six calls on one state; L = 4099 misaligns every row but one in four, offset 1 misaligns the best rows against
    aligned delta rows.  up_every 2, down_every 3, clamps [5e-6, 1.5e-5] around alpha0 = 1e-5."""
    B, milli, up_every, down_every, up, down, lo, hi = 7, 500, 2, 3, 1.2, 0.8, 5e-6, 1.5e-5
    rng = np.random.default_rng(L + offset)
    delta = torch.from_numpy(rng.standard_normal((B, L)).astype(np.float32)).cuda()
    best, alpha, bloss, balpha = Guarded((B, L), offset=offset), Guarded((B,)), Guarded((B,)), Guarded((B,))
    bstep, step = Guarded((B,), torch.int32), Guarded((1,), torch.int32)
    pattern = (np.arange(B * L, dtype=np.float32).reshape(B, L) % 251) - 1000.0
    best.t.copy_(torch.from_numpy(pattern))
    alpha.t.fill_(1e-5)
    bloss.t.fill_(float("inf"))
    balpha.t.fill_(9.0)
    bstep.t.fill_(-1)
    step.t.fill_(0)
    S = (0, 2, 2) if targeted else (2, 2, 2)          # a success in the mode under test
    F_ = (1, 2, 2) if targeted else (0, 2, 2)         # a failure in it
    E = (0, 0, 0)                                     # an empty reference: a failure in both
    nan = float("nan")
    # per call: (counts, loss) of rows 0 .. 6
    #   row 0  succeeds always, its loss falls: a keep at every call; alpha rises at n = 2, 4 and 6 (to the upper clamp)
    #   row 1  succeeds always with one loss: kept once, every later call is a tie and keeps the earlier delta
    #   row 2  succeeds always, its loss rises: kept at call 0 only
    #   row 3  succeeds always with a NaN loss: never kept, alpha still rises
    #   row 4  fails always: alpha falls at n = 3 and n = 6 (to the lower clamp); nothing else of it is ever written
    #   row 5  fails, except at call 2 (n = 3, off the success period: kept, alpha not moved) — its failure at n = 6 lowers alpha
    #   row 6  an empty reference, then successes from call 3 on with a NaN, a high and a lower loss
    calls = [([S, S, S, S, F_, F_, E], [9.0, 3.0, 1.0, nan, 1.0, 1.0, 1.0]),
             ([S, S, S, S, F_, F_, E], [8.0, 3.0, 2.0, nan, 0.5, 1.0, 1.0]),
             ([S, S, S, S, F_, S, E], [7.0, 3.0, 3.0, nan, 0.2, 4.0, 1.0]),
             ([S, S, S, S, F_, F_, S], [6.0, 3.0, 4.0, nan, 0.1, 0.1, nan]),
             ([S, S, S, S, F_, F_, S], [5.0, 3.0, 5.0, nan, 0.1, 0.1, 6.0]),
             ([S, S, S, S, F_, F_, S], [4.0, 3.0, 6.0, nan, 0.1, 0.1, 2.0])]
    ref = (alpha.t.cpu().numpy(), pattern.copy(), bloss.t.cpu().numpy(), balpha.t.cpu().numpy(), bstep.t.cpu().numpy(), 0)
    for i, (cnt, ls) in enumerate(calls):
        delta.add_(1.0)                                                # another delta every call
        delta_np = delta.cpu().numpy()
        counts = torch.tensor(cnt, dtype=torch.int32, device="cuda")
        loss = torch.tensor(ls, dtype=torch.float32, device="cuda")
        assert SR.success(cnt, targeted, milli).tolist() == [c == S for c in cnt]
        with record_launches() as names:
            st = _anneal_call(delta, counts, loss, targeted, milli, up_every, down_every, up, down, lo, hi, alpha.t, best.t, bloss.t,
                              balpha.t, bstep.t, step.t)
        torch.cuda.synchronize()
        assert st == _lib.PAA_OK and names == ["paa_clip_anneal"]
        ref = AR.clip_anneal(delta_np, cnt, ls, targeted, milli, up_every, down_every, up, down, lo, hi, *ref)
        got = (alpha.t.cpu().numpy(), best.t.cpu().numpy(), bloss.t.cpu().numpy(), balpha.t.cpu().numpy(), bstep.t.cpu().numpy(),
               int(step.t.item()))
        for name, g_, r_ in zip(("alpha", "best", "best_loss", "best_alpha", "best_step"), got, ref):
            assert np.array_equal(np.asarray(g_).view(np.uint32), np.asarray(r_).view(np.uint32)), (name, i, g_, r_)
        assert got[5] == ref[5] == i + 1                               # the counter advances on the device
        assert np.array_equal(delta.cpu().numpy(), delta_np)           # delta is read only
        for g_ in (best, alpha, bloss, balpha, bstep, step):
            g_.check()
    f = np.float32
    a0 = f(1e-5)
    assert int(step.t.item()) == 6
    # what the construction promises, from the reference's state
    al, bl, ba, bs = ref[0], ref[2], ref[3], ref[4]
    assert bs.tolist() == [5, 0, 0, -1, -1, 2, 5]
    assert bl[:3].tolist() == [4.0, 3.0, 1.0] and np.isinf(bl[3]) and np.isinf(bl[4]) and bl[5] == 4.0 and bl[6] == 2.0
    assert al[0] == f(hi) and al[3] == f(hi)                           # 1e-5 -> 1.2e-5 -> 1.44e-5 -> 1.728e-5, clamped to 1.5e-5
    assert al[4] == f(max(f(f(a0 * f(down)) * f(down)), f(lo))) == f(f(a0 * f(down)) * f(down))       # 6.4e-6: above the clamp
    assert ba[0] == f(f(a0 * f(up)) * f(up)) and ba[1] == a0 and ba[5] == a0 and ba[3] == 9.0 and ba[4] == 9.0
    # rows 3 and 4 were never flagged: the sentinel pattern stands
    for b in (3, 4):
        assert np.array_equal(best.t[b].cpu().numpy(), pattern[b])
    # the lower clamp: three more failing periods take row 4 from 6.4e-6 to 5e-6 and keep it there
    for i in range(6, 15):
        cnt = [F_] * B
        st = _anneal_call(delta, torch.tensor(cnt, dtype=torch.int32, device="cuda"), torch.ones(B, device="cuda"), targeted, milli,
                          up_every, down_every, up, down, lo, hi, alpha.t, best.t, bloss.t, balpha.t, bstep.t, step.t)
        assert st == _lib.PAA_OK
        ref = AR.clip_anneal(delta.cpu().numpy(), cnt, np.ones(B), targeted, milli, up_every, down_every, up, down, lo, hi, *ref)
    torch.cuda.synchronize()
    assert np.array_equal(alpha.t.cpu().numpy().view(np.uint32), ref[0].view(np.uint32)) and int(step.t.item()) == 15
    assert float(alpha.t[4]) == f(lo) and np.array_equal(bstep.t.cpu().numpy(), bs)
    for g_ in (best, alpha, bloss, balpha, bstep, step):
        g_.check()


def test_clip_anneal_argument_contract():
    """Every refusal comes before any launch: the outputs keep their bits."""
    B, L = 2, 64
    delta = torch.randn(B, L, device="cuda")
    counts = torch.tensor([[2, 2, 2], [2, 2, 2]], dtype=torch.int32, device="cuda")       # both rows would succeed and be kept
    loss = torch.zeros(B, device="cuda")
    out = {k: Guarded(s, d) for k, (s, d) in dict(alpha=((B,), torch.float32), best=((B, L), torch.float32),
                                                  bloss=((B,), torch.float32), balpha=((B,), torch.float32),
                                                  bstep=((B,), torch.int32), step=((1,), torch.int32)).items()}
    for g in out.values():
        g.t.view(torch.int32).fill_(7)
    ok = dict(delta=delta, counts=counts, loss=loss, targeted=0, milli=500, up_every=1, down_every=1, up=1.2, down=0.8, lo=1e-7,
              hi=1e-3, **{k: g.t for k, g in out.items()})

    def call(**kw):
        a = {**ok, **kw}
        b, l = a.get("B", B), a.get("L", L)
        return _lib.lib().paa_clip_anneal(_lib.ptr(a["delta"]), b, l, _lib.ptr(a["counts"]), _lib.ptr(a["loss"]), a["targeted"],
                                          a["milli"], a["up_every"], a["down_every"], a["up"], a["down"], a["lo"], a["hi"],
                                          _lib.ptr(a["alpha"]), _lib.ptr(a["best"]), _lib.ptr(a["bloss"]), _lib.ptr(a["balpha"]),
                                          _lib.ptr(a["bstep"]), _lib.ptr(a["step"]), _lib.stream_ptr())
    inf, nan = float("inf"), float("nan")
    bad = [{k: None} for k in ("delta", "counts", "loss", "alpha", "best", "bloss", "balpha", "bstep", "step")]
    bad += [dict(B=0), dict(B=-1), dict(B=65536), dict(L=0), dict(milli=0), dict(milli=-5), dict(up_every=0), dict(down_every=0),
            dict(up_every=-2), dict(up=1.0), dict(up=0.5), dict(up=inf), dict(up=nan), dict(down=0.0), dict(down=1.0), dict(down=-0.5),
            dict(down=nan), dict(lo=0.0), dict(lo=-1e-7), dict(lo=nan), dict(lo=2e-3), dict(hi=inf), dict(hi=nan)]
    with record_launches() as names:
        for kw in bad:
            assert call(**kw) == _lib.PAA_ERR_ARG, kw
            assert b"paa_clip_anneal" in _lib.lib().paa_last_error()
    torch.cuda.synchronize()
    assert names.count("paa_clip_anneal") == len(bad) and set(names) == {"paa_clip_anneal", "paa_last_error"}
    for g in out.values():
        assert bool((g.t.view(torch.int32) == 7).all())
        g.check()
    out["alpha"].t.fill_(1e-5)
    out["bloss"].t.fill_(float("inf"))
    assert call(lo=1e-5, hi=1e-5) == _lib.PAA_OK and call(up=1.0001, down=0.9999) == _lib.PAA_OK       # the closed ends, just inside
    torch.cuda.synchronize()
    assert int(out["step"].t.item()) == 9


# ---- 3. the stepper against a host-driven loop ----------------------------------------------------------------------------------
ALPHA0 = 1e-5          # the order of max|grad CTC| / max|grad l| DESIGN.md §6d measured on these models


def _case(arch, B, L, opt):
    a = A.tiny("group", False) if arch == "group" else A.tiny("layer", True)
    args = _args(ALPHA0)
    args.optimizer_type = opt
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = opgd.make_labels(["ab cd", "hello", "a b c"][:B], args, B)
    d0 = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * 1e-2).cuda()
    return m, args, clean, labels, d0


class HostLoop:
    """The step of the schedule's stepper with the decision taken on the host: the same entries in the same order, the ids and the
    l_b downloaded, anneal_ref applied, the alphas uploaded for the next paa_masking_loss_rows."""

    def __init__(self, m, args, clean, labels, d0, refs, cfg, bound_scale=None):
        self.m, self.args, self.clean, self.refs, self.cfg, self.labels = m, args, clean, refs, cfg, labels
        self.B, self.L = d0.shape
        self.delta = d0.clone()
        self.direction = +1 if args.attack_mode == "untargeted" else -1
        self.alpha = np.full(self.B, np.float32(args.masking_loss_alpha), dtype=np.float32)
        self.best = np.zeros((self.B, self.L), dtype=np.float32)
        self.best_loss = np.full(self.B, np.inf, dtype=np.float32)
        self.best_alpha = np.zeros(self.B, dtype=np.float32)
        self.best_step = np.full(self.B, -1, dtype=np.int32)
        self.step_no = 0
        self.history = []                    # per step: (success flags, l_b, alpha_b the step ran under)
        self.adam = args.optimizer_type == "adam"
        if self.adam:
            self.opt = torch.optim.Adam([torch.nn.Parameter(self.delta)], lr=args.lr)
            self.m1, self.m2 = torch.zeros_like(self.delta), torch.zeros_like(self.delta)
            self.t = 0
        self.prm = [runtime.params_of(args, n) for n in str(args.norm_type).split("+")]
        self.mask_prm = runtime.params_of(args, "masking")
        self.proj = runtime.get_proj(args, "cuda", self.B, self.L)
        self.bound_scale = bound_scale
        self.loss_rows, self.loss_sum = torch.zeros(self.B, device="cuda"), torch.zeros(1, device="cuda")

    def step(self):
        lib, st, B, L, c = _lib.lib(), _lib.stream_ptr(), self.B, self.L, self.cfg
        r = self.m.fwd_bwd(self.clean, self.delta, self.labels, self.direction)
        al = torch.from_numpy(self.alpha.copy()).cuda()
        _lib.check(lib.paa_masking_loss_rows(self.proj.h, self.mask_prm, _lib.ptr(self.delta), B, _lib.ptr(self.clean), B, L, _lib.ptr(al),
                                             B, _lib.ptr(r["grad"]), _lib.ptr(self.loss_rows), _lib.ptr(self.loss_sum), None, st))
        torch.cuda.synchronize()
        counts = _host_counts(_hyp(self.m, r["logits"], B), self.refs)
        loss = self.loss_rows.cpu().numpy()
        self.history.append((SR.success(counts, c.targeted, c.wer_milli), loss.copy(), self.alpha.copy()))
        self.alpha, self.best, self.best_loss, self.best_alpha, self.best_step, self.step_no = AR.clip_anneal(
            self.delta.cpu().numpy(), counts, loss, c.targeted, c.wer_milli, c.up_every, c.down_every, c.up, c.down, c.alpha_min,
            c.alpha_max, self.alpha, self.best, self.best_loss, self.best_alpha, self.best_step, self.step_no)
        if not self.adam:
            _lib.check(lib.paa_sign_step(_lib.ptr(self.delta), _lib.ptr(r["grad"]), float(self.args.lr), B * L, st))
        else:
            g = self.opt.param_groups[0]
            self.t += 1
            scal = torch.tensor(pgd.adam_scalars(g["lr"], g["betas"][0], g["betas"][1], float(self.t)), dtype=torch.float32).cuda()
            b1, b2 = g["betas"]
            _lib.check(lib.paa_adam_step(_lib.ptr(self.delta), _lib.ptr(r["grad"]), -1.0, _lib.ptr(self.m1), _lib.ptr(self.m2),
                                         _lib.ptr(scal), float(1 - b1), float(b2), float(1 - b2), float(g["eps"]), None, B * L, st))
        for prm in self.prm:
            if self.bound_scale is None:
                _lib.check(lib.paa_project_rows(self.proj.h, prm, _lib.ptr(self.delta), _lib.ptr(self.delta), B, _lib.ptr(self.clean), L,
                                                st))
            else:
                _lib.check(lib.paa_project_rows_scaled(self.proj.h, prm, _lib.ptr(self.delta), _lib.ptr(self.delta), B,
                                                       _lib.ptr(self.clean), L, _lib.ptr(self.bound_scale), st))
        torch.cuda.synchronize()

    def same_as(self, delta, stp, where):
        B = self.B
        torch.cuda.synchronize()
        eq = lambda t, a: np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))
        found = self.best_step >= 0
        assert torch.equal(delta, self.delta), (where, "delta")
        assert eq(stp.alpha_rows[:B], self.alpha), (where, "alpha_rows", stp.alpha_rows[:B].tolist(), self.alpha)
        assert eq(stp.best_loss[:B], self.best_loss), (where, "best_loss", stp.best_loss[:B].tolist(), self.best_loss)
        assert eq(stp.best_step[:B], self.best_step), (where, "best_step")
        assert int(stp.anneal_step.item()) == self.step_no, (where, "step")
        assert np.array_equal(stp.best_alpha[:B].cpu().numpy()[found], self.best_alpha[found]), (where, "best_alpha")
        assert np.array_equal(stp.best[:B].cpu().numpy()[found], self.best[found]), (where, "best")


def _anneal_stepper(m, args, L, d, refs, cfg, bound_scale=None):
    opt = torch.optim.Adam([d], lr=args.lr) if args.optimizer_type == "adam" else None
    stp = ClipStepper(m, args, L, optimizer=opt, device_wer=True, anneal=cfg, bound_scale=bound_scale)
    stp.set_refs(loss_helpers.encode_refs(refs))
    stp.anneal_reset(d.shape[0])
    return stp


def _table(host, tag):
    print(f"{tag}: step | success | l_b | alpha_b the step ran under")
    for i, (ok, loss, al) in enumerate(host.history):
        print(f"  {i} | {ok.astype(int).tolist()} | {[f'{v:.4e}' for v in loss]} | {[f'{v:.3e}' for v in al]}")
    print(f"  best_step {host.best_step.tolist()} best_loss {host.best_loss.tolist()} best_alpha {host.best_alpha.tolist()} "
          f"alpha {host.alpha.tolist()}")


def _run_stepper_case(arch, opt, targeted, steps=7):
    B, L = 3, 16000
    m, args, clean, labels, d0 = _case(arch, B, L, opt)
    if targeted:
        args.attack_mode = "targeted"
        cfg = AnnealConfig(1.2, 0.8, 2, 3, 1e-7, 1e-3, 500, True)
        refs = [OTHER] * B                               # a target no hypothesis equals: nobody ever succeeds
    else:
        cfg = AnnealConfig(1.2, 0.8, 2, 1, 1e-7, 1e-3, 500, False)
        r0 = m.fwd_bwd(clean, d0, labels, +1, want_grad=False)
        torch.cuda.synchronize()
        own = _hyp(m, r0["logits"], B)[1]
        print(f"{arch} {opt}: hypotheses of the start {_hyp(m, r0['logits'], B)}")
        assert own.split(), "the model's own hypothesis is empty: no reference to fail against"
        refs = [OTHER, own, OTHER]                       # clips 0 and 2 succeed at every step, clip 1 fails at step 0
    host = HostLoop(m, args, clean, labels, d0, refs, cfg)
    de = torch.nn.Parameter(d0.clone()) if opt == "adam" else d0.clone()
    ded = de.data if opt == "adam" else de
    stp = _anneal_stepper(m, args, L, de, refs, cfg)
    with record_launches() as names:
        stp.step(ded, clean, labels)
    upd = "paa_adam_step" if opt == "adam" else "paa_sign_step"
    assert names.index("paa_masking_loss_rows") < names.index("paa_wer_counts") < names.index("paa_clip_anneal") < names.index(upd) \
        < names.index("paa_project_rows")
    assert "paa_masking_loss" not in names and "paa_clip_search" not in names and "paa_project_rows_scaled" not in names
    host.step()
    host.same_as(ded, stp, (arch, opt, targeted, "eager", 0))
    for i in range(1, steps):
        stp.step(ded, clean, labels)
        host.step()
        host.same_as(ded, stp, (arch, opt, targeted, "eager", i))
    _table(host, f"{arch} {opt} {'targeted' if targeted else 'untargeted'}")
    ok = np.array([h[0] for h in host.history])
    al = np.array([h[2] for h in host.history] + [host.alpha])          # alpha before step i; the last row: after the last step
    loss = np.array([h[1] for h in host.history])
    assert (loss > 0).all(), "the masking term is in play at every step"
    f = np.float32
    if targeted:
        assert not ok.any() and (host.best_step == -1).all() and np.isinf(host.best_loss).all()
        a1 = f(f(ALPHA0) * f(0.8))
        # n = 3 and n = 6: every alpha falls after steps 2 and 5, and nowhere else
        assert (al[:3] == f(ALPHA0)).all() and (al[3:6] == a1).all() and (al[6:] == f(a1 * f(0.8))).all()
    else:
        assert ok[:, 0].all() and ok[:, 2].all() and not ok[0, 1]
        assert al[2, 0] == f(f(ALPHA0) * f(1.2)) and al[2, 2] == al[2, 0] and al[1, 0] == f(ALPHA0)      # the raise at n = 2
        assert al[1, 1] == f(f(ALPHA0) * f(0.8))                                                        # the lowering at n = 1
        assert host.best_step[0] >= 0 and host.best_step[2] >= 0
        for b in (0, 2):                                 # the kept loss is the least of the successful steps, its first occurrence
            assert host.best_loss[b] == loss[:, b].min() and host.best_step[b] == int(loss[:, b].argmin())
            assert host.best_alpha[b] == al[host.best_step[b], b]
    # captured and replayed: the warm-up step is undone for delta and the schedule's buffers
    dg = torch.nn.Parameter(d0.clone()) if opt == "adam" else d0.clone()
    dgd = dg.data if opt == "adam" else dg
    stg = _anneal_stepper(m, args, L, dg, refs, cfg)
    g, _ = stg.capture(dgd, clean, labels)
    torch.cuda.synchronize()
    assert torch.equal(dgd, d0) and int(stg.anneal_step.item()) == 0 and bool((stg.best_step[:B] == -1).all())
    assert bool((stg.alpha_rows[:B] == f(ALPHA0)).all()) and bool(torch.isinf(stg.best_loss[:B]).all())
    host2 = HostLoop(m, args, clean, labels, d0, refs, cfg)
    for i in range(steps):
        g.replay()
        host2.step()
        host2.same_as(dgd, stg, (arch, opt, targeted, "replay", i))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
               for a, b in zip(host.history, host2.history))
    return m, args, clean, labels, d0, refs, cfg


@pytest.mark.parametrize("arch,opt", [("group", "pgd"), ("layer", "adam")])
def test_stepper_vs_host_loop_untargeted(arch, opt):
    _run_stepper_case(arch, opt, False)


def test_stepper_vs_host_loop_targeted_nobody_succeeds():
    _run_stepper_case("group", "pgd", True)


def test_stepper_with_fixed_bound_scales():
    B, L, steps = 3, 16000, 7
    m, args, clean, labels, d0 = _case("group", B, L, "pgd")
    cfg = AnnealConfig(1.2, 0.8, 2, 1, 1e-7, 1e-3, 500, False)
    refs = [OTHER] * B
    scale = torch.tensor([1.0, 0.5, 0.25], device="cuda")
    host = HostLoop(m, args, clean, labels, d0, refs, cfg, bound_scale=scale.clone())
    d = d0.clone()
    stp = _anneal_stepper(m, args, L, d, refs, cfg, bound_scale=scale)
    for i in range(steps):
        with record_launches() as names:
            stp.step(d, clean, labels)
        assert "paa_project_rows_scaled" in names and "paa_project_rows" not in names
        host.step()
        host.same_as(d, stp, ("bound_scale", i))
        lim = np.float32(args.linf_size) * scale.cpu().numpy() * (1 + ROW_TOL)
        assert bool((d.abs().amax(dim=1).cpu().numpy() <= lim).all()), (i, d.abs().amax(dim=1).tolist(), lim)
    assert torch.equal(scale, torch.tensor([1.0, 0.5, 0.25], device="cuda"))       # nothing writes it
    assert float(d[0].abs().max()) > float(np.float32(args.linf_size) * 0.5)       # the rows do use their own bounds
    assert (host.best_step >= 0).all()
    with pytest.raises(ValueError, match="device tensor"):
        ClipStepper(m, args, L, device_wer=True, anneal=cfg, bound_scale=[1.0, 0.5, 0.25])


# ---- 4. the schedule off ---------------------------------------------------------------------------------------------------------
def test_schedule_off_launches_nothing_new():
    B, L = 3, 16000
    m, args, clean, labels, d0 = _case("group", B, L, "pgd")
    a, b = d0.clone(), d0.clone()
    st = ClipStepper(m, args, L)                                       # alpha0 > 0, no schedule: as built before it existed
    assert st.anneal is None and st.bound_scale is None and not hasattr(st, "alpha_rows") and not hasattr(st, "best")
    with record_launches() as names:
        for _ in range(3):
            st.step(a, clean, labels)
    assert names.count("paa_masking_loss") == 3 and names.count("paa_project_rows") == 3
    assert not {"paa_masking_loss_rows", "paa_clip_anneal", "paa_clip_search", "paa_project_rows_scaled"} & set(names)
    # the step it has always been: forward / backward, the scalar masking loss, sign step, row projection
    alpha = torch.tensor([ALPHA0], dtype=torch.float32, device="cuda")
    lr = torch.zeros(B, device="cuda")
    for _ in range(3):
        r = m.fwd_bwd(clean, b, labels, +1)
        _lib.check(_lib.lib().paa_masking_loss(st.proj.h, runtime.params_of(args, "masking"), _lib.ptr(b), B, _lib.ptr(clean), B, L,
                                               _lib.ptr(alpha), _lib.ptr(r["grad"]), _lib.ptr(lr), None, None, _lib.stream_ptr()))
        _lib.check(_lib.lib().paa_sign_step(_lib.ptr(b), _lib.ptr(r["grad"]), float(args.lr), B * L, _lib.stream_ptr()))
        _lib.check(_lib.lib().paa_project_rows(st.proj.h, runtime.params_of(args), _lib.ptr(b), _lib.ptr(b), B, _lib.ptr(clean), L,
                                               _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(st.mask_rows[:B], lr) and bool((lr > 0).all())
    with pytest.raises(RuntimeError, match="without an alpha schedule"):
        st.anneal_reset(B)


# ---- 5. the entry point -----------------------------------------------------------------------------------------------------------
ENTRY = ["--norm_type", "linf", "--linf_size", "0.05", "--pgd_steps", "8", "--optimizer_type", "pgd", "--lr", "1e-3",
         "--num_items_to_inspect", "0", "--masking_loss_alpha", "1e-5", "--alpha_search", "qin", "--alpha_up_every", "2"]
A_MIN, A_MAX = 1e-5 / 100.0, 1e-5 * 100.0


def _check_anneal_records(res):
    clips = res["clips"]
    assert len(clips) >= 2
    for c in clips:
        assert all(k in c for k in ("alpha_found", "alpha_step", "best_masking_loss", "best_alpha", "last_alpha", "final_masking_loss")), c
        assert c["alpha_found"] == (c["alpha_step"] >= 0)
        assert np.float32(A_MIN) <= np.float32(c["last_alpha"]) <= np.float32(A_MAX), c
        assert np.float32(A_MIN) <= np.float32(c["best_alpha"]) <= np.float32(A_MAX), c
        if c["alpha_found"]:
            rel = abs(c["final_masking_loss"] - c["best_masking_loss"]) / max(abs(c["best_masking_loss"]), 1e-30)
            print(f"clip {c['index']}: best_masking_loss {c['best_masking_loss']!r} final_masking_loss {c['final_masking_loss']!r} "
                  f"rel {rel:.1e} bit-equal {c['final_masking_loss'] == c['best_masking_loss']}")
            assert rel <= 1e-6, c
        else:
            assert np.isnan(c["best_masking_loss"]) and c["best_alpha"] == c["last_alpha"], c
    s = res["summary"]
    hit = [c for c in clips if c["alpha_found"]]
    assert s["alpha_success_rate"] == len(hit) / len(clips)
    if hit:
        assert s["mean_best_masking_loss"] == sum(c["best_masking_loss"] for c in hit) / len(hit)
    return hit


def test_entry_point_alpha_search_alone(tmp_path):
    logs = str(tmp_path / "logs")
    p = _run_entry(ENTRY + ["--logs_dir", logs])
    assert p.wait(900) == 0
    res = _results(logs)
    hit = _check_anneal_records(res)
    print(json.dumps(res["summary"]))
    # an untrained model's transcript shares no word with the references: every clip succeeds at every step
    assert len(hit) == len(res["clips"])
    assert all("found" not in c and "stage1_masking_loss" not in c for c in res["clips"])
    # eight successful steps with up_every 2: four raises
    f = np.float32
    a = f(1e-5)
    for _ in range(4):
        a = f(a * f(1.2))
    assert all(f(c["last_alpha"]) == a for c in res["clips"]), [c["last_alpha"] for c in res["clips"]]


def test_entry_point_two_stage(tmp_path):
    logs = str(tmp_path / "logs")
    p = _run_entry(ENTRY + ["--bound_search", "shrink", "--stage1_steps", "3", "--logs_dir", logs])
    assert p.wait(900) == 0
    res = _results(logs)
    _check_anneal_records(res)
    print(json.dumps(res["summary"]))
    found = [c for c in res["clips"] if c["found"]]
    assert found, "stage 1 found nobody: the case shows nothing"
    for c in res["clips"]:
        assert all(k in c for k in ("found", "found_step", "bound_scale", "last_scale", "stage1_masking_loss")), c
        assert c["found_step"] < 3 and c["alpha_step"] < 5
        assert c["linf"] <= float(np.float32(0.05) * np.float32(c["bound_scale"])) * (1 + ROW_TOL), c
        if c["found"]:
            assert c["alpha_found"], c                   # the delta that enters stage 2 is judged at its step 0 by the same forward
            assert c["best_masking_loss"] <= c["stage1_masking_loss"], c
    s = res["summary"]
    assert list(s)[-4:] == ["success_rate", "mean_bound_scale", "alpha_success_rate", "mean_best_masking_loss"]


def test_entry_point_two_ranks_equal_one_two_stage(tmp_path):
    common = ENTRY + ["--bound_search", "shrink", "--stage1_steps", "3"]
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    p = _run_entry(common + ["--logs_dir", one])
    assert p.wait(900) == 0
    port = str(_free_port())
    ps = [_run_entry(common + ["--logs_dir", two], dict(WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                                                        MASTER_PORT=port, PAA_DIST_BACKEND="gloo"), batch_size=2) for r in range(2)]
    assert [q.wait(900) for q in ps] == [0, 0]
    r1, r2 = _results(one), _results(two)
    assert [c["index"] for c in r1["clips"]] == [c["index"] for c in r2["clips"]]
    for c1, c2 in zip(r1["clips"], r2["clips"]):
        for k in ("found", "found_step", "bound_scale", "last_scale", "clean_wer", "adv_wer", "alpha_found", "alpha_step", "best_alpha",
                  "last_alpha"):
            assert c1[k] == c2[k], (k, c1[k], c2[k])
        for k in ("clean_ctc", "final_ctc", "l2", "linf", "snr_db", "best_masking_loss", "stage1_masking_loss", "final_masking_loss"):
            assert abs(c1[k] - c2[k]) <= 1e-5 * max(abs(c1[k]), 1e-6) or (np.isnan(c1[k]) and np.isnan(c2[k])), (k, c1[k], c2[k])
    assert r1["summary"]["alpha_success_rate"] == r2["summary"]["alpha_success_rate"]
    assert r1["summary"]["success_rate"] == r2["summary"]["success_rate"]


@pytest.mark.parametrize("extra,msg", [
    (["--masking_loss_alpha", "0"], "--alpha_search qin needs --masking_loss_alpha > 0"),
    (["--stage1_steps", "3"], "--stage1_steps applies to the two-stage run"),
])
def test_entry_point_refusals(tmp_path, extra, msg):
    import subprocess
    import sys
    from test_gpu_search import ROOT
    cmd = [sys.executable, "-m", "paa_amd.attack_clips", "--arch", "tiny", "--device", "cuda", "--audio_seconds", "0.5", "--batch_size", "4",
           "--steps_per_epoch", "2", "--small_data", "--silent", *ENTRY, "--logs_dir", str(tmp_path / "logs"), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and msg in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "logs"))                   # refused before the run directory is made
