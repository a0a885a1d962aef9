"""-m gpu: the per-clip bound search.  paa_project_rows_scaled row by row against oracle.projections with the size
scaled in the args; paa_clip_search bit for bit against tests/search_ref.py; the device-search ClipStepper (eager, then captured and
replayed) against a loop that runs the same entries but decides on the host; the entry point with --bound_search shrink."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import search_ref as SR
from gpu_util import PROJ_ARGS, SCALES, branch as _branch, record_launches, rel_err, rows_input as _rows_input, \
    scaled_args as _scaled_args, with_ as _with
from oracle import pgd as opgd, projections as OP
from oracle.gen_cases import cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils import clip_attack, pgd
from paa_amd.training_utils.clip_attack import ClipStepper, SearchConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = ["l2", "linf", "snr", "tv", "fletcher_munson", "max_phon", "min_max_freqs+tv"]
ROW_TOL = 2e-5          # the project's own bound for row projections (test_gpu_clip_attack.test_project_rows_vs_oracle)


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


def _scaled(pr, prm, src, dst, rows, clean, L, scale):
    _lib.check(_lib.lib().paa_project_rows_scaled(pr.h, prm, _lib.ptr(src), _lib.ptr(dst), rows, _lib.ptr(clean), L, _lib.ptr(scale),
                                                  _lib.stream_ptr()))


def _check_scaled_vs_oracle(norm, args, L, rows, seen):
    spl = OP.spl_thresh_tensor(args)
    parts = norm.split("+")
    src_np, clean_np = _rows_input(rows, L)
    src, clean = torch.from_numpy(src_np).cuda(), torch.from_numpy(clean_np).cuda()
    scale = torch.from_numpy(SCALES[:rows].copy()).cuda()
    pr = runtime.get_proj(args, src.device, rows, L)
    pr.set_spl_thresh(spl.cuda())
    got, inplace = src.clone(), src.clone()
    for n in parts:
        prm = runtime.params_of(_with(args, norm_type=n))
        out = torch.empty_like(got)
        _scaled(pr, prm, got, out, rows, clean, L, scale)
        got = out
        _scaled(pr, prm, inplace, inplace, rows, clean, L, scale)
    torch.cuda.synchronize()
    assert torch.equal(inplace, got), (norm, L, rows)                  # in place == out of place
    g = got.cpu().numpy()
    assert np.isfinite(g).all()
    worst = 0.0
    for r in range(rows):
        ref, c = torch.from_numpy(src_np[r:r + 1]), torch.from_numpy(clean_np[r:r + 1])
        with torch.no_grad():
            for n in parts:
                a = _scaled_args(args, n, SCALES[r])
                moved, dist = _branch(n, ref, c, a)
                assert dist > 1e-4, ("a row on its projection's branch", norm, n, L, r, dist)
                if moved is not None:
                    seen.add((n, moved))
                ref = OP.perturbation_constraint(ref, c, a, spl)
        worst = max(worst, rel_err(g[r], ref.numpy()[0]))
    print(f"{norm} n_fft={args.n_fft} L={L} rows={rows}: max row rel err vs the oracle at the scaled size {worst:.2e}")
    assert worst < ROW_TOL, (norm, L, rows, worst)


@pytest.mark.parametrize("norm", NORMS)
def test_scaled_rows_vs_oracle(norm):
    args = cli_to_args(norm, PROJ_ARGS)
    seen = set()
    for L in (16000, 24001):
        for rows in (1, 3, 5):
            _check_scaled_vs_oracle(norm, args, L, rows, seen)
    # the norms with a row-level "over the bound?" branch, the composite through its tv part; max_phon and min_max_freqs clip
    # bin by bin and have no such branch
    for n in norm.split("+"):
        if n in ("l2", "linf", "snr", "tv", "fletcher_munson"):
            assert (n, True) in seen and (n, False) in seen, (norm, n, seen)


@pytest.mark.parametrize("norm", ["fletcher_munson", "max_phon"])
def test_scaled_rows_vs_oracle_generic_frames(norm):
    """n_fft 512, hop 128: the generic one-frame-per-workgroup kernels (k_fm_finalize with one group per row, the OP_PHON frame kernel)."""
    args = cli_to_args(norm, PROJ_ARGS + ["--n_fft", "512", "--hop_length", "128", "--win_length", "512"])
    seen = set()
    _check_scaled_vs_oracle(norm, args, 16000, 3, seen)
    if norm == "fletcher_munson":
        assert seen == {(norm, True), (norm, False)}


@pytest.mark.parametrize("norm", NORMS)
def test_null_and_unit_scales_are_the_unscaled_call(norm):
    args = cli_to_args(norm, PROJ_ARGS)
    spl = OP.spl_thresh_tensor(args)
    rows = 3
    for L in (16000, 24001):
        src_np, clean_np = _rows_input(rows, L)
        src, clean = torch.from_numpy(src_np).cuda(), torch.from_numpy(clean_np).cuda()
        ones = torch.ones(rows, device="cuda")
        pr = runtime.get_proj(args, src.device, rows, L)
        pr.set_spl_thresh(spl.cuda())
        for in_place in (False, True):
            outs = []
            for scale in ("plain", None, ones):
                cur = src.clone()
                for n in norm.split("+"):
                    prm = runtime.params_of(_with(args, norm_type=n))
                    dst = cur if in_place else torch.empty_like(cur)
                    if isinstance(scale, str):
                        _lib.check(_lib.lib().paa_project_rows(pr.h, prm, _lib.ptr(cur), _lib.ptr(dst), rows, _lib.ptr(clean), L,
                                                               _lib.stream_ptr()))
                    else:
                        _scaled(pr, prm, cur, dst, rows, clean, L, scale)
                    cur = dst
                outs.append(cur)
            torch.cuda.synchronize()
            assert torch.equal(outs[1], outs[0]), (norm, L, in_place, "NULL scale")
            assert torch.equal(outs[2], outs[0]), (norm, L, in_place, "unit scales")
        # one row with a unit scale takes the row launches: the bits of the one-row call all the same
        one, c1 = src[:1].contiguous(), clean[:1].contiguous()
        a_, b_ = one.clone(), one.clone()
        for n in norm.split("+"):
            prm = runtime.params_of(_with(args, norm_type=n))
            _lib.check(_lib.lib().paa_project_rows(pr.h, prm, _lib.ptr(a_), _lib.ptr(a_), 1, _lib.ptr(c1), L, _lib.stream_ptr()))
            _scaled(pr, prm, b_, b_, 1, c1, L, ones)
        torch.cuda.synchronize()
        assert torch.equal(a_, b_), (norm, L, "one row")


def test_bad_device_scales_act_as_one():
    """NaN, inf, 0 and a negative value on the device are treated as 1.0f: no NaN rows."""
    rows, L = 4, 16000
    src_np, clean_np = _rows_input(rows, L)
    src, clean = torch.from_numpy(src_np).cuda(), torch.from_numpy(clean_np).cuda()
    bad = torch.tensor([float("nan"), float("inf"), 0.0, -0.5], device="cuda")
    for norm in ("l2", "linf", "snr", "tv", "fletcher_munson", "max_phon"):
        args = cli_to_args(norm, PROJ_ARGS)
        pr = runtime.get_proj(args, src.device, rows, L)
        pr.set_spl_thresh(OP.spl_thresh_tensor(args).cuda())
        prm = runtime.params_of(args)
        a_, b_ = torch.empty_like(src), torch.empty_like(src)
        _scaled(pr, prm, src, a_, rows, clean, L, bad)
        _scaled(pr, prm, src, b_, rows, clean, L, torch.ones(rows, device="cuda"))
        torch.cuda.synchronize()
        assert torch.isfinite(a_).all() and torch.equal(a_, b_), norm


def test_masking_with_a_scale_is_a_bad_norm():
    args = cli_to_args("masking", [])
    rows, L = 2, 16000
    src_np, clean_np = _rows_input(rows, L)
    src, clean = torch.from_numpy(src_np).cuda(), torch.from_numpy(clean_np).cuda()
    pr = runtime.get_proj(args, src.device, rows, L)
    before = src.clone()
    with pytest.raises(ValueError, match="masking norm takes no bound scale"):
        _scaled(pr, runtime.params_of(args), src, src, rows, clean, L, torch.ones(rows, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(src, before)
    # without a scale the entry is paa_project_rows, the masking norm included
    a_, b_ = src.clone(), src.clone()
    _scaled(pr, runtime.params_of(args), a_, a_, rows, clean, L, None)
    _lib.check(_lib.lib().paa_project_rows(pr.h, runtime.params_of(args), _lib.ptr(b_), _lib.ptr(b_), rows, _lib.ptr(clean), L,
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(a_, b_) and not torch.equal(a_, before)


# ---- paa_clip_search alone ------------------------------------------------------------------------------------------------------
SENT = -0x21524111         # 0xDEADBEEF read as int32; as float32 -6.26e18


class Guarded:
    """A float32 / int32 device tensor between two guard blocks of a sentinel pattern; ``offset`` elements shift its base."""

    def __init__(self, shape, dtype=torch.float32, offset=0):
        self.n, self.g = int(np.prod(shape)), 256 + int(offset)
        self.full = torch.full((self.n + 512 + int(offset),), SENT, dtype=torch.int32, device="cuda")
        self.t = self.full[self.g:self.g + self.n].view(dtype).view(tuple(shape))

    def check(self):
        assert bool((self.full[:self.g] == SENT).all()) and bool((self.full[self.g + self.n:] == SENT).all()), "guard overwritten"


def _search_call(delta, counts, targeted, milli, shrink, floor, scale, best, bscale, bstep, step):
    B, L = delta.shape
    _lib.check(_lib.lib().paa_clip_search(_lib.ptr(delta), B, L, _lib.ptr(counts), int(targeted), int(milli), float(shrink),
                                          float(floor), _lib.ptr(scale), _lib.ptr(best), _lib.ptr(bscale), _lib.ptr(bstep),
                                          _lib.ptr(step), _lib.stream_ptr()))


@pytest.mark.parametrize("targeted", [False, True])
@pytest.mark.parametrize("L,offset", [(4096, 0), (4099, 0), (4096, 1)])
def test_clip_search_vs_reference(L, offset, targeted):
    """B = 5 rows; L = 4099 misaligns every row but one in four, offset 1 misaligns the best rows against aligned delta rows."""
    B, shrink, floor, milli = 5, 0.5, 0.2, 500
    rng = np.random.default_rng(L + offset)
    delta_np = rng.standard_normal((B, L)).astype(np.float32)
    delta = torch.from_numpy(delta_np).cuda()
    best, scale, bscale = Guarded((B, L), offset=offset), Guarded((B,)), Guarded((B,))
    bstep, step = Guarded((B,), torch.int32), Guarded((1,), torch.int32)
    pattern = (np.arange(B * L, dtype=np.float32).reshape(B, L) % 251) - 1000.0
    best.t.copy_(torch.from_numpy(pattern))
    scale.t.copy_(torch.tensor([1.0, 0.7, 0.5, 0.3, 0.21]))
    bscale.t.fill_(9.0)
    bstep.t.fill_(-1)
    step.t.fill_(41)
    # (errors, reference words, hypothesis words) per call: successes and failures mixed, in both modes
    r0 = (0, 2, 2) if targeted else (2, 2, 2)                          # row 0 succeeds in every call, in its mode
    calls = [[r0, (1, 2, 2), (0, 0, 0), (2, 4, 1), (1, 3, 3)],
             [r0, (0, 3, 3), (5, 0, 5), (1, 4, 4), (3, 3, 0)],
             [r0, (2, 2, 2), (0, 1, 1), (4, 4, 4), (0, 3, 3)]]
    ref = (scale.t.cpu().numpy(), pattern.copy(), bscale.t.cpu().numpy(), bstep.t.cpu().numpy(), 41)
    hit_rows, miss_rows = set(), set(range(B))
    for i, cnt in enumerate(calls):
        delta.add_(1.0)                                                # another delta every call
        delta_np = delta.cpu().numpy()
        counts = torch.tensor(cnt, dtype=torch.int32, device="cuda")
        with record_launches() as names:
            _search_call(delta, counts, targeted, milli, shrink, floor, scale.t, best.t, bscale.t, bstep.t, step.t)
        torch.cuda.synchronize()
        assert names == ["paa_clip_search"]
        ok = SR.success(cnt, targeted, milli)
        hit_rows |= set(np.nonzero(ok)[0].tolist())
        miss_rows -= set(np.nonzero(ok)[0].tolist())
        ref = SR.clip_search(delta_np, cnt, targeted, milli, shrink, floor, *ref)
        got = (scale.t.cpu().numpy(), best.t.cpu().numpy(), bscale.t.cpu().numpy(), bstep.t.cpu().numpy(), int(step.t.item()))
        for name, g_, r_ in zip(("scale", "best", "best_scale", "best_step"), got, ref):
            assert np.array_equal(np.asarray(g_).view(np.uint32), np.asarray(r_).view(np.uint32)), (name, i, g_, r_)
        assert got[4] == ref[4] == 42 + i                              # the counter advances on the device
        assert np.array_equal(delta.cpu().numpy(), delta_np)           # delta is read only
        for g_ in (best, scale, bscale, bstep, step):
            g_.check()
    assert hit_rows and miss_rows                                      # both kinds of row occurred
    for b in miss_rows:                                                # never flagged: the sentinel pattern and the scalars stand
        assert np.array_equal(best.t[b].cpu().numpy(), pattern[b]) and float(bscale.t[b]) == 9.0 and int(bstep.t[b]) == -1
    # row 0 succeeded in all three calls: 1 -> 0.5 -> 0.25 -> the floor 0.2
    assert float(scale.t[0]) == np.float32(0.2) and float(bscale.t[0]) == 0.25 and int(bstep.t[0]) == 43


def test_argument_contract():
    """Every refusal of both entries comes before any launch: the outputs keep their bits."""
    B, L = 2, 64
    delta = torch.randn(B, L, device="cuda")
    counts = torch.tensor([[2, 2, 2], [2, 2, 2]], dtype=torch.int32, device="cuda")       # both rows would succeed
    out = {k: Guarded(s, d) for k, (s, d) in dict(scale=((B,), torch.float32), best=((B, L), torch.float32),
                                                  bscale=((B,), torch.float32), bstep=((B,), torch.int32),
                                                  step=((1,), torch.int32)).items()}
    for g in out.values():
        g.t.view(torch.int32).fill_(7)
    ok = dict(delta=delta, counts=counts, targeted=0, milli=500, shrink=0.8, floor=0.01,
              **{k: g.t for k, g in out.items()})

    def call(**kw):
        a = {**ok, **kw}
        d = a["delta"]
        b, l = (a.get("B"), a.get("L"))
        return _lib.lib().paa_clip_search(_lib.ptr(d), B if b is None else b, L if l is None else l, _lib.ptr(a["counts"]),
                                          a["targeted"], a["milli"], a["shrink"], a["floor"], _lib.ptr(a["scale"]), _lib.ptr(a["best"]),
                                          _lib.ptr(a["bscale"]), _lib.ptr(a["bstep"]), _lib.ptr(a["step"]), _lib.stream_ptr())
    bad = [{k: None} for k in ("delta", "counts", "scale", "best", "bscale", "bstep", "step")]
    bad += [dict(B=0), dict(L=0), dict(B=-1), dict(shrink=0.0), dict(shrink=1.0), dict(shrink=-0.5), dict(shrink=float("nan")),
            dict(floor=0.0), dict(floor=1.0001), dict(floor=float("nan")), dict(milli=0), dict(milli=-5)]
    with record_launches() as names:
        for kw in bad:
            assert call(**kw) == _lib.PAA_ERR_ARG, kw
            assert b"paa_clip_search" in _lib.lib().paa_last_error()
    torch.cuda.synchronize()
    assert names.count("paa_clip_search") == len(bad) and set(names) == {"paa_clip_search", "paa_last_error"}
    for g in out.values():
        assert bool((g.t.view(torch.int32) == 7).all())
        g.check()
    assert call(floor=1.0) == _lib.PAA_OK and call(shrink=0.999) == _lib.PAA_OK        # the closed end of (0, 1], just inside (0, 1)
    torch.cuda.synchronize()
    assert int(out["step"].t.item()) == 9
    # paa_project_rows_scaled: the null / size / need-clean contract of paa_project_rows, the destination untouched
    args = cli_to_args("snr", PROJ_ARGS)
    pr = runtime.get_proj(args, "cuda", 2, 16000)
    prm = runtime.params_of(args)
    src = torch.randn(2, 16000, device="cuda")
    dst, ones = Guarded((2, 16000)), torch.ones(2, device="cuda")
    dst.t.view(torch.int32).fill_(7)
    L_ = _lib.lib()
    st = _lib.stream_ptr()
    sp, dp, cp, op = _lib.ptr(src), _lib.ptr(dst.t), _lib.ptr(src), _lib.ptr(ones)
    assert L_.paa_project_rows_scaled(None, prm, sp, dp, 2, cp, 16000, op, st) == _lib.PAA_ERR_ARG
    assert L_.paa_project_rows_scaled(pr.h, None, sp, dp, 2, cp, 16000, op, st) == _lib.PAA_ERR_ARG
    assert L_.paa_project_rows_scaled(pr.h, prm, None, dp, 2, cp, 16000, op, st) == _lib.PAA_ERR_ARG
    assert L_.paa_project_rows_scaled(pr.h, prm, sp, None, 2, cp, 16000, op, st) == _lib.PAA_ERR_ARG
    assert L_.paa_project_rows_scaled(pr.h, prm, sp, dp, 0, cp, 16000, op, st) == _lib.PAA_ERR_SIZE
    assert L_.paa_project_rows_scaled(pr.h, prm, sp, dp, pr.max_batch + 1, cp, 16000, op, st) == _lib.PAA_ERR_SIZE
    assert L_.paa_project_rows_scaled(pr.h, prm, sp, dp, 2, cp, pr.max_len + 1, op, st) == _lib.PAA_ERR_SIZE
    assert L_.paa_project_rows_scaled(pr.h, prm, sp, dp, 2, None, 16000, op, st) == _lib.PAA_ERR_NEED_CLEAN
    torch.cuda.synchronize()
    assert bool((dst.t.view(torch.int32) == 7).all())
    dst.check()
    with pytest.raises(ValueError, match="finite and > 0"):
        clip_attack.project_rows(src, src.clone(), args, scale=[1.0, float("nan")])


# ---- the stepper against a host-driven loop -------------------------------------------------------------------------------------
STEP_FLAGS = {"linf": ["--linf_size", "0.05", "--lr", "0.01"], "snr": ["--snr_db", "10", "--lr", "0.01"]}
OTHER = "zzz qqq jjj"          # a reference no hypothesis of these models equals: an untargeted success at every step


HD64 = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256)      # head dim 64: the fused attention path lengths need


def _case(arch, norm, B, L, opt, lengths=None):
    kw = HD64 if lengths is not None else {}
    a = A.tiny("group", False, **kw) if arch == "group" else A.tiny("layer", True, **kw)
    args = cli_to_args(norm, STEP_FLAGS[norm])
    args.device, args.optimizer_type = "cuda", opt
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = opgd.make_labels(["ab cd", "hello", "a b c"][:B], args, B)
    d0 = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * 1e-3).cuda()
    if lengths is not None:
        m.set_lengths(lengths)
        clip_attack.mask_tail_rows(d0, lengths)
    return m, args, clean, labels, d0


def _hyp(m, logits, B):
    frames = m.frame_counts(B) if m.lengths_on else None
    ids = loss_helpers.argmax_ids(logits, frames, int(m.arch.pad_token_id))
    return [t.strip().lower() for t in loss_helpers.greedy_decode_ids(ids.cpu().tolist())]


def _host_counts(hyp, refs):
    out = []
    for h, r in zip(hyp, loss_helpers.clean_transcripts(refs)):
        e, w = loss_helpers.wer_counts([h], [r])
        out.append((e, w, len(h.split())))
    return out


class HostLoop:
    """The step of the search stepper with the decision taken on the host: the same entries in the same order, the ids downloaded
    and decoded with loss_helpers, search_ref applied, the scales uploaded for paa_project_rows_scaled."""

    def __init__(self, m, args, clean, labels, d0, refs, cfg):
        self.m, self.args, self.clean, self.refs, self.cfg = m, args, clean, refs, cfg
        self.labels = labels
        self.B, self.L = d0.shape
        self.delta = d0.clone()
        self.direction = +1 if args.attack_mode == "untargeted" else -1
        self.scale = np.ones(self.B, dtype=np.float32)
        self.best = np.zeros((self.B, self.L), dtype=np.float32)
        self.best_scale = np.ones(self.B, dtype=np.float32)
        self.best_step = np.full(self.B, -1, dtype=np.int32)
        self.step_no = 0
        self.history = []                    # per step: the success flags
        self.adam = args.optimizer_type == "adam"
        if self.adam:
            self.opt = torch.optim.Adam([torch.nn.Parameter(self.delta)], lr=args.lr)
            self.m1, self.m2 = torch.zeros_like(self.delta), torch.zeros_like(self.delta)
            self.t = 0
        self.prm = [runtime.params_of(args, n) for n in str(args.norm_type).split("+")]
        self.proj = runtime.get_proj(args, "cuda", self.B, self.L)

    def step(self):
        lib, st, B, L = _lib.lib(), _lib.stream_ptr(), self.B, self.L
        r = self.m.fwd_bwd(self.clean, self.delta, self.labels, self.direction)
        torch.cuda.synchronize()
        counts = _host_counts(_hyp(self.m, r["logits"], B), self.refs)
        self.history.append(SR.success(counts, self.cfg.targeted, self.cfg.wer_milli))
        self.scale, self.best, self.best_scale, self.best_step, self.step_no = SR.clip_search(
            self.delta.cpu().numpy(), counts, self.cfg.targeted, self.cfg.wer_milli, self.cfg.shrink, self.cfg.floor_scale, self.scale,
            self.best, self.best_scale, self.best_step, self.step_no)
        if not self.adam:
            _lib.check(lib.paa_sign_step(_lib.ptr(self.delta), _lib.ptr(r["grad"]), float(self.args.lr), B * L, st))
        else:
            g = self.opt.param_groups[0]
            self.t += 1
            scal = torch.tensor(pgd.adam_scalars(g["lr"], g["betas"][0], g["betas"][1], float(self.t)), dtype=torch.float32).cuda()
            b1, b2 = g["betas"]
            _lib.check(lib.paa_adam_step(_lib.ptr(self.delta), _lib.ptr(r["grad"]), -1.0, _lib.ptr(self.m1), _lib.ptr(self.m2),
                                         _lib.ptr(scal), float(1 - b1), float(b2), float(1 - b2), float(g["eps"]), None, B * L, st))
        sc = torch.from_numpy(self.scale.copy()).cuda()
        for prm in self.prm:
            _lib.check(lib.paa_project_rows_scaled(self.proj.h, prm, _lib.ptr(self.delta), _lib.ptr(self.delta), B, _lib.ptr(self.clean),
                                                   L, _lib.ptr(sc), st))
            if self.m.lengths_on:
                _lib.check(lib.paa_mask_tail_rows(_lib.ptr(self.delta), B, L, _lib.ptr(self.m._lengths), st))
        torch.cuda.synchronize()

    def same_as(self, delta, stp, where):
        B = self.B
        torch.cuda.synchronize()
        assert torch.equal(delta, self.delta), (where, "delta")
        assert np.array_equal(stp.scale[:B].cpu().numpy(), self.scale), (where, "scale", stp.scale[:B].tolist(), self.scale)
        assert np.array_equal(stp.best_step[:B].cpu().numpy(), self.best_step), (where, "best_step")
        assert int(stp.search_step.item()) == self.step_no, (where, "step")
        found = self.best_step >= 0
        assert np.array_equal(stp.best_scale[:B].cpu().numpy()[found], self.best_scale[found]), (where, "best_scale")
        assert np.array_equal(stp.best[:B].cpu().numpy()[found], self.best[found]), (where, "best")


def _search_stepper(m, args, L, d, refs, cfg):
    opt = torch.optim.Adam([d], lr=args.lr) if args.optimizer_type == "adam" else None
    stp = ClipStepper(m, args, L, optimizer=opt, device_wer=True, search=cfg)
    stp.set_refs(loss_helpers.encode_refs(refs))
    stp.search_reset(d.shape[0])
    return stp


def _bound_ok(norm, args, best, clean, s):
    """best satisfies the bound of ``norm`` at scale s, within the projection tolerance."""
    if norm == "linf":
        return float(best.abs().max()) <= float(np.float32(args.linf_size) * np.float32(s)) * (1 + ROW_TOL)
    cur = 10 * np.log10(float((clean.double() ** 2).mean()) / (float((best.double() ** 2).mean()) + 1e-12))
    return cur >= args.snr_db - 20 * np.log10(float(s)) - 20 * np.log10(1 + ROW_TOL)       # ROW_TOL in amplitude, as dB


def _run_stepper_case(arch, norm, opt, lengths=None, steps=6):
    B, L = 3, 16000
    m, args, clean, labels, d0 = _case(arch, norm, B, L, opt, lengths)
    cfg = SearchConfig(0.8, 0.01, 500, False)
    # clip 1 is judged against the model's own hypothesis for the delta it starts from: it fails until the attack changes a word
    r0 = m.fwd_bwd(clean, d0, labels, +1, want_grad=False)
    torch.cuda.synchronize()
    own = _hyp(m, r0["logits"], B)[1]
    print(f"{arch} {norm} {opt}: hypotheses of the start {_hyp(m, r0['logits'], B)}")
    assert own.split(), "the model's own hypothesis is empty: no reference to fail against"
    refs = [OTHER, own, OTHER]
    host = HostLoop(m, args, clean, labels, d0, refs, cfg)
    # eager
    de = torch.nn.Parameter(d0.clone()) if opt == "adam" else d0.clone()
    stp = _search_stepper(m, args, L, de, refs, cfg)
    with record_launches() as names:
        stp.step(de.data if opt == "adam" else de, clean, labels)
    assert names.index("paa_wer_counts") < names.index("paa_clip_search") < names.index(
        "paa_adam_step" if opt == "adam" else "paa_sign_step") < names.index("paa_project_rows_scaled")
    assert "paa_project_rows" not in names
    host.step()
    host.same_as(de.data if opt == "adam" else de, stp, (arch, norm, opt, "eager", 0))
    for i in range(1, steps):
        stp.step(de.data if opt == "adam" else de, clean, labels)
        host.step()
        host.same_as(de.data if opt == "adam" else de, stp, (arch, norm, opt, "eager", i))
    hist = np.array(host.history)
    print(f"{arch} {norm} {opt}: success per step and clip\n{hist.astype(int)}\nscales {host.scale} best_step {host.best_step}")
    assert hist[0, 0], "clip 0 succeeds at step 0"
    assert not hist[0, 1] and hist[1:, 1].any(), "clip 1 fails first and succeeds later"
    assert hist[:, 2].sum() >= 2, "clip 2 succeeds at two different steps"
    assert not hist.all() and hist.any()
    # the invariant: every found best row satisfies its norm's bound at best_scale
    best, bscale = stp.best[:B].clone(), stp.best_scale[:B].cpu().numpy()
    for b in np.nonzero(host.best_step >= 0)[0]:
        n_b = L if lengths is None else int(lengths[b])
        assert _bound_ok(norm, args, best[b, :n_b], clean[b, :n_b], bscale[b]), (arch, norm, opt, b, bscale[b])
        if lengths is not None:
            assert bool((best[b, n_b:] == 0).all()), "a best row keeps the zero tail"
    # captured and replayed: the warm-up step is undone for delta and the search buffers
    dg = torch.nn.Parameter(d0.clone()) if opt == "adam" else d0.clone()
    stg = _search_stepper(m, args, L, dg, refs, cfg)
    dgd = dg.data if opt == "adam" else dg
    g, _ = stg.capture(dgd, clean, labels)
    torch.cuda.synchronize()
    assert torch.equal(dgd, d0) and int(stg.search_step.item()) == 0 and bool((stg.best_step[:B] == -1).all())
    assert bool((stg.scale[:B] == 1).all())
    host2 = HostLoop(m, args, clean, labels, d0, refs, cfg)
    for i in range(steps):
        g.replay()
        host2.step()
        host2.same_as(dgd, stg, (arch, norm, opt, "replay", i))
    assert np.array_equal(np.array(host2.history), hist)
    return stp


@pytest.mark.parametrize("opt", ["pgd", "adam"])
@pytest.mark.parametrize("norm", ["linf", "snr"])
@pytest.mark.parametrize("arch", ["group", "layer"])
def test_stepper_vs_host_loop(arch, norm, opt):
    _run_stepper_case(arch, norm, opt)


def test_stepper_true_lengths_vs_host_loop():
    _run_stepper_case("group", "linf", "pgd", lengths=torch.tensor([16000, 12345, 9001]))


def test_search_off_launches_nothing_new():
    B, L = 3, 16000
    m, args, clean, labels, d0 = _case("group", "snr", B, L, "pgd")
    a, b = d0.clone(), d0.clone()
    st = ClipStepper(m, args, L)                                       # as built before the search existed: positional, no config
    assert st.search is None and not hasattr(st, "best")
    with record_launches() as names:
        for _ in range(3):
            st.step(a, clean, labels)
    assert "paa_clip_search" not in names and "paa_project_rows_scaled" not in names and names.count("paa_project_rows") == 3
    # the step it has always been: forward / backward, sign step, row projection through the plain entries
    for _ in range(3):
        r = m.fwd_bwd(clean, b, labels, +1)
        _lib.check(_lib.lib().paa_sign_step(_lib.ptr(b), _lib.ptr(r["grad"]), float(args.lr), B * L, _lib.stream_ptr()))
        _lib.check(_lib.lib().paa_project_rows(st.proj.h, runtime.params_of(args), _lib.ptr(b), _lib.ptr(b), B, _lib.ptr(clean), L,
                                               _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="without a bound search"):
        st.search_reset(B)


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def _run_entry(extra, env_extra=None, batch_size=4):
    """A fresh child process per rank (no exec of a process that has initialised the GPU)."""
    env = dict(os.environ, **(env_extra or {}))
    cmd = [sys.executable, "-m", "paa_amd.attack_clips", "--arch", "tiny", "--device", "cuda", "--audio_seconds", "0.5",
           "--batch_size", str(batch_size), "--steps_per_epoch", "2", "--small_data", "--silent", *extra]
    return subprocess.Popen(cmd, cwd=ROOT, env=env)


def _results(logs):
    path = None
    for d, _, files in os.walk(logs):
        if "clip_results.json" in files:
            path = os.path.join(d, "clip_results.json")
    assert path, logs
    return json.load(open(path))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _check_records(res, targeted, thr=0.5, floor=0.01):
    clips = res["clips"]
    assert len(clips) >= 2
    for c in clips:
        assert all(k in c for k in ("found", "found_step", "bound_scale", "last_scale")), c
        assert floor <= c["last_scale"] <= c["bound_scale"] <= 1.0, c
        assert c["found"] == (c["found_step"] >= 0)
        if c["found"]:
            # the re-evaluated record agrees with the step's own decision
            assert (c["target_wer"] == 0) if targeted else (c["adv_wer"] >= thr), c
            assert c["last_scale"] < c["bound_scale"] or c["bound_scale"] == floor, c
        else:
            assert c["bound_scale"] == c["last_scale"] == 1.0, c
    s = res["summary"]
    hit = [c for c in clips if c["found"]]
    assert s["success_rate"] == len(hit) / len(clips)
    if hit:
        assert s["mean_bound_scale"] == sum(c["bound_scale"] for c in hit) / len(hit)
    else:
        assert np.isnan(s["mean_bound_scale"])
    return hit


ENTRY_FLAGS = ["--norm_type", "snr", "--snr_db", "20", "--pgd_steps", "8", "--optimizer_type", "pgd", "--lr", "1e-3",
               "--num_items_to_inspect", "0", "--bound_search", "shrink"]


def _start_hypotheses(batch_size=4):
    """What the entry point's model writes for every clip of its first batch under the perturbation the attack starts from: the
    entry point's own loaders, model, initial draw and projection, the forward of the step, the host decode."""
    from paa_amd import attack_clips
    from paa_amd.training_utils import build
    args = attack_clips.create_arg_parser().parse_args(
        ["--arch", "tiny", "--device", "cuda", "--audio_seconds", "0.5", "--batch_size", str(batch_size), "--steps_per_epoch", "2",
         "--small_data", "--silent", *ENTRY_FLAGS])
    batches, length = attack_clips.split_batches(args, 1)
    x, texts, idx = attack_clips.clip_batches(batches, 0, 1)[0][:3]
    model, processor = build.load_model(args, max_batch=len(texts), length=length)
    assert processor is None
    x = x.to("cuda", torch.float32).contiguous()
    delta = torch.from_numpy(clip_attack.init_rows(x.shape[1], idx, int(args.seed))).cuda()
    clip_attack.project_rows(delta, x, args, None, build.init_phon_threshold_tensor(args))
    r = model.fwd_bwd(x, delta, loss_helpers.make_labels(texts, None, args, len(texts)), -1, want_grad=False)
    torch.cuda.synchronize()
    hyp = _hyp(model, r["logits"], len(texts))
    del model
    return hyp, idx


@pytest.mark.parametrize("mode", ["untargeted", "targeted"])
def test_entry_point_with_bound_search(tmp_path, mode):
    logs = str(tmp_path / "logs")
    extra = ["--attack_mode", mode]
    if mode == "targeted":
        # the target is what the model writes for clip 0 under the perturbation it starts from, so that clip's attack has
        # succeeded at step 0 by construction: the targeted route (target rows as references, the targeted flag, the re-scoring
        # at direction -1) is exercised with a success in it
        hyp, idx = _start_hypotheses()
        print(f"targeted: start hypotheses {hyp}")
        assert hyp[0].split() and idx[0] == 0
        extra += ["--target", hyp[0], "--target_reps", "1"]
    p = _run_entry(ENTRY_FLAGS + ["--logs_dir", logs, *extra])
    assert p.wait(900) == 0
    res = _results(logs)
    hit = _check_records(res, mode == "targeted")
    print(f"{mode}: {json.dumps(res['summary'])}")
    if mode == "untargeted":
        # an untrained model's transcript shares no word with the references: every clip falls, at the first step it is asked
        assert len(hit) == len(res["clips"]) and all(c["snr_db"] > 19.0 for c in res["clips"])
    else:
        assert len(hit) >= 1 and res["clips"][0]["found"] and res["clips"][0]["target_wer"] == 0, res["clips"]
        assert hyp[0] != hyp[1] or len(hit) >= 2


def test_entry_point_two_ranks_equal_one_with_bound_search(tmp_path):
    common = ["--norm_type", "snr", "--snr_db", "20", "--pgd_steps", "4", "--optimizer_type", "pgd", "--lr", "1e-3",
              "--num_items_to_inspect", "0", "--bound_search", "shrink"]
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    p = _run_entry(common + ["--logs_dir", one])
    assert p.wait(900) == 0
    port = str(_free_port())
    ps = [_run_entry(common + ["--logs_dir", two], dict(WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                                                        MASTER_PORT=port, PAA_DIST_BACKEND="gloo"), batch_size=2) for r in range(2)]
    assert [q.wait(900) for q in ps] == [0, 0]
    r1, r2 = _results(one), _results(two)
    _check_records(r1, False)
    assert [c["index"] for c in r1["clips"]] == [c["index"] for c in r2["clips"]]
    for c1, c2 in zip(r1["clips"], r2["clips"]):
        for k in ("found", "found_step", "bound_scale", "last_scale", "clean_wer", "adv_wer"):
            assert c1[k] == c2[k], (k, c1[k], c2[k])
        for k in ("clean_ctc", "final_ctc", "l2", "linf", "snr_db"):
            assert abs(c1[k] - c2[k]) <= 1e-5 * max(abs(c1[k]), 1e-6), (k, c1[k], c2[k])
    assert r1["summary"]["success_rate"] == r2["summary"]["success_rate"]
