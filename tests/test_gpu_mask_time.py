"""-m gpu: temporal masking of the masking threshold.  theta' of the device equals tests/mask_time_ref.spread32 of
the device's own theta bit for bit; projections and the masking loss are held to the references fed theta', with the tolerances of
tests/test_gpu_masking.py and tests/test_gpu_masking_loss.py; empty tables give back the bits of a context that never had the mode;
the device steps replay as they run eagerly; the runners name the run after the mode and write its keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mask_time_ref as MT
import masking_ref as MR
import test_gpu_masking_loss as TL          # _call / _check_rows: the loss term's own comparison, tolerances and ambiguous-bin rule
from oracle import pgd as opgd
from oracle.gen_cases import PGD_TEXTS, cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.core.masking import masking_loss, masking_threshold
from paa_amd.model import PaaModel
from paa_amd.training_utils.clip_attack import ClipStepper
from paa_amd.training_utils.pgd import PgdStepper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 513
SENT = -0x21524111                           # 0xDEADBEEF as float32: -6.26e18
TIMES = [(200.0, 20.0), (320.0, 0.0), (0.0, 20.0)]
# (2, 600): T = 3, every table longer than the clip; (2, 4096): T = 17 < J_post; (3, 16000): T = 63, two time tiles of the kernel
SHAPES = ["2x600", "2x4096", "3x16000", "burst"]


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    runtime._PROJ.clear()
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


def _args(times=None, norm="masking", **kw):
    a = cli_to_args(norm, [])
    a.masking_margin_db, a.device = 0.0, "cuda"
    if times is not None:
        a.masking_post_ms, a.masking_pre_ms = times
    for k, v in kw.items():
        setattr(a, k, v)
    return a


_CLEAN = {}


def _clean(name):
    """The clean clips of a case as float32 (B, L), computed once."""
    if name not in _CLEAN:
        if name == "burst":
            x = MT.burst_clip().astype(np.float32)[None]
        else:
            B, L = (int(v) for v in name.split("x"))
            x = synth.clean_audio(B, L, seed=7 if L < 8000 else 3)
        x.setflags(write=False)
        _CLEAN[name] = x
    return _CLEAN[name]


def _dev(x_np):
    return torch.from_numpy(np.array(x_np, dtype=np.float32, order="C")).cuda()          # a copy: the cached clips stay read-only


_OFF = {}


def _theta_off(name):
    """(theta, pmax, psd) of the case with the mode off, device tensors, computed once and left alone."""
    if name not in _OFF:
        x = _dev(_clean(name))
        _OFF[name] = masking_threshold(x, _args(), psd=True)
        torch.cuda.synchronize()
    return _OFF[name]


class Guarded:
    """A float32 device tensor with a guard block of the sentinel pattern in front of it and behind it (tests/test_gpu_rows.py)."""

    def __init__(self, shape):
        shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(shape))
        self.g = -(-max(shape[-1], 256) // 64) * 64
        self.full = torch.full((self.n + 2 * self.g,), SENT, dtype=torch.int32, device="cuda")
        self.t = self.full[self.g:self.g + self.n].view(torch.float32).view(shape)

    def check(self):
        assert bool((self.full[:self.g] == SENT).all()) and bool((self.full[self.g + self.n:] == SENT).all()), "guard block overwritten"


def _threshold_into(pr, x, theta, pmax=None, psd=None):
    B, L = x.shape
    _lib.check(_lib.lib().paa_masking_threshold(pr.h, _lib.ptr(x), B, L, _lib.ptr(psd), _lib.ptr(theta), _lib.ptr(pmax), _lib.stream_ptr()))


@pytest.mark.parametrize("times", TIMES, ids=lambda t: f"{t[0]:g}-{t[1]:g}")
@pytest.mark.parametrize("name", SHAPES)
def test_threshold_is_the_reference_spread_bit_for_bit(name, times):
    x_np = _clean(name)
    x = _dev(x_np)
    B, L = x.shape
    T = 1 + L // 256
    th_off, pm_off, psd_off = _theta_off(name)
    post, pre = MT.tables(*times)
    want = torch.from_numpy(MT.spread32(th_off.cpu().numpy(), post, pre)).cuda()
    args = _args(times)
    pr = runtime.get_proj(args, "cuda", B, L)
    assert pr is not runtime.get_proj(_args(), "cuda", B, L)                 # the mode is part of the context key
    out, pmax, psd = Guarded((B, T, F)), Guarded((B,)), Guarded((B, T, F))
    _threshold_into(pr, x, out.t, pmax.t, psd.t)
    torch.cuda.synchronize()
    for g in (out, pmax, psd):
        g.check()
    assert torch.equal(out.t, want), (name, times, int((out.t != want).sum()))
    assert torch.equal(pmax.t, pm_off) and torch.equal(psd.t, psd_off)       # what pass 2 writes beside theta is untouched
    assert bool((out.t >= th_off).all())
    if times[0] > 0 and name != "2x600":
        assert bool((out.t > th_off).any())                                  # post-masking raises cells of every longer clip
    again = Guarded((B, T, F))
    _threshold_into(pr, x, again.t)                                          # no d_pmax, no d_psd
    th_pub, pm_pub = masking_threshold(x, args)
    torch.cuda.synchronize()
    again.check()
    assert torch.equal(again.t, out.t) and torch.equal(th_pub, out.t) and torch.equal(pm_pub, pm_off)


def test_clips_under_the_reflect_padding_are_refused_as_before():
    """(1, 256) would be T = 2, but every entry of the library needs L > n_fft / 2 = 512 for the reflect padding: the clip is
    refused with the mode on exactly as with it off, so T = 3 (L = 600) is the shortest plane the spread can meet."""
    x = torch.zeros(1, 256, device="cuda")
    th = torch.empty(1, 2, F, device="cuda")
    for times in (None, TIMES[0]):
        pr = runtime.get_proj(_args(times), "cuda", 1, 4096)
        st = _lib.lib().paa_masking_threshold(pr.h, _lib.ptr(x), 1, 256, None, _lib.ptr(th), None, _lib.stream_ptr())
        assert st == _lib.PAA_ERR_SIZE


def _noise(B, L, amp=1e-2):
    return (np.stack([synth.normal(synth.key_of(f"mask{b}", 3), L) for b in range(B)]) * amp).astype(np.float32)


def _proj_rows(pr, prm, src, clean):
    B, L = src.shape
    out = torch.empty_like(src)
    _lib.check(_lib.lib().paa_project_rows(pr.h, prm, _lib.ptr(src), _lib.ptr(out), B, _lib.ptr(clean), L, _lib.stream_ptr()))
    return out


def _proj_universal(pr, prm, src, clean):
    B, L = clean.shape
    out = torch.empty_like(src)
    _lib.check(_lib.lib().paa_project_to(pr.h, prm, _lib.ptr(src), _lib.ptr(out), 1, _lib.ptr(clean), B, L, _lib.stream_ptr()))
    return out


def _loss(pr, prm, d, clean):
    rows, L = d.shape
    B = clean.shape[0]
    g, lr = torch.zeros_like(d), torch.empty(B, device="cuda")
    _lib.check(_lib.lib().paa_masking_loss(pr.h, prm, _lib.ptr(d), rows, _lib.ptr(clean), B, L, None, _lib.ptr(g), _lib.ptr(lr), None, None,
                                           _lib.stream_ptr()))
    return g, lr


def _everything(pr, prm, d, clean):
    """Threshold, per-clip and universal projection, per-clip and universal loss and gradient of one context."""
    B, L = clean.shape
    th = torch.empty(B, 1 + L // 256, F, device="cuda")
    _threshold_into(pr, clean, th)
    out = [th, _proj_rows(pr, prm, d, clean), _proj_universal(pr, prm, d[:1].contiguous(), clean),
           *_loss(pr, prm, d, clean), *_loss(pr, prm, d[:1].contiguous(), clean)]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["2x4096", "3x16000"])
def test_empty_tables_give_back_the_parents_bits(name):
    x_np = _clean(name)
    B, L = x_np.shape
    clean, d = _dev(x_np), torch.from_numpy(_noise(B, L, 3e-2)).cuda()
    off, on = _args(), _args(TIMES[0])
    prm = runtime.params_of(off)
    want = _everything(runtime.get_proj(off, "cuda", B, L), prm, d, clean)             # a context that never saw the setter
    pr = runtime.Proj("cuda", 1024, 256, 1024, 16000, B, L, spread=MT.tables(*TIMES[0]))          # a context of this test's own
    used = _everything(pr, prm, d, clean)
    assert not torch.equal(used[0], want[0]) and not torch.equal(used[1], want[1]) and not torch.equal(used[4], want[4])
    _lib.check(_lib.lib().paa_proj_set_masking_spread(pr.h, 0, None, 0, None))
    back = _everything(pr, prm, d, clean)
    for i, (a, b) in enumerate(zip(back, want)):
        assert torch.equal(a, b), (name, i)
    post, pre = MT.tables(*TIMES[0])                                                  # and on again: the bits of the first use
    _lib.check(_lib.lib().paa_proj_set_masking_spread(pr.h, len(post), post.ctypes.data, len(pre), pre.ctypes.data))
    for i, (a, b) in enumerate(zip(_everything(pr, prm, d, clean), used)):
        assert torch.equal(a, b), (name, i)


def test_context_key_and_growth():
    on, off = _args(TIMES[0]), _args()
    a = runtime.get_proj(on, "cuda", 1, 4096)
    assert a is runtime.get_proj(on, "cuda", 1, 4096) and a is not runtime.get_proj(off, "cuda", 1, 4096)
    assert a is not runtime.get_proj(_args(TIMES[1]), "cuda", 1, 4096)
    big = runtime.get_proj(on, "cuda", max(a.max_batch, 1) + 1, a.max_len + 256)      # a grown context keeps its tables
    assert big is not a and all(np.array_equal(p, q) for p, q in zip(big.spread, MT.tables(*TIMES[0])))
    x = _dev(_clean("2x4096"))
    th, _ = masking_threshold(x, on)
    torch.cuda.synchronize()
    assert torch.equal(th, torch.from_numpy(MT.spread32(_theta_off("2x4096")[0].cpu().numpy(), *MT.tables(*TIMES[0]))).cuda())


@pytest.mark.parametrize("times", TIMES[:2], ids=lambda t: f"{t[0]:g}-{t[1]:g}")
@pytest.mark.parametrize("name", ["2x600", "2x4096", "3x16000"])
def test_projections_vs_reference(name, times):
    """paa_project_rows and the universal projection against masking_ref.project under the bound of theta' (the device's own theta',
    checked bit for bit above): the tolerances of tests/test_gpu_masking.py, 2e-5 of the reference's largest sample."""
    x_np = _clean(name)
    B, L = x_np.shape
    d_np = _noise(B, L)
    clean, d = _dev(x_np), torch.from_numpy(d_np).cuda()
    args = _args(times)
    prm = runtime.params_of(args)
    pr = runtime.get_proj(args, "cuda", B, L)
    got = _proj_rows(pr, prm, d, clean)
    uni = _proj_universal(pr, prm, d[:1].contiguous(), clean)
    theta, pmax = masking_threshold(clean, args)
    torch.cuda.synchronize()
    th, pm, g = theta.cpu().numpy(), pmax.cpu().numpy(), got.cpu().numpy()
    for b in range(B):
        ref = MR.project(d_np[b], MR.bound(th[b], pm[b]), L)
        e = np.abs(g[b] - ref).max() / np.abs(ref).max()
        print(f"{name} {times} row {b}: rel err {e:.2e}")
        assert e < 2e-5, (name, times, b, e)
    A_min = np.min(np.stack([MR.bound(th[b], pm[b]) for b in range(B)]), axis=0)
    ref = MR.project(d_np[0], A_min, L)
    e = np.abs(uni.cpu().numpy()[0] - ref).max() / np.abs(ref).max()
    print(f"{name} {times} universal: rel err {e:.2e}")
    assert e < 2e-5, (name, times, e)


@pytest.mark.parametrize("name,amp", [("3x16000", 3e-2), ("2x4096", 3e-2)])
def test_masking_loss_vs_reference(name, amp):
    """The loss term and its gradient against tests/masking_loss_ref.py fed theta': test_gpu_masking_loss's own comparison."""
    x_np = _clean(name)
    B, L = x_np.shape
    d_np = _noise(B, L, amp)
    clean, d = _dev(x_np), torch.from_numpy(d_np).cuda()
    args = _args(TIMES[0])
    th, pm = TL._device_threshold(args, clean)
    uni = TL._call(args, d[:1].contiguous(), clean)
    TL._check_rows(f"uni {name}", d_np[:1], [list(range(B))], th, pm, uni, 0.05)
    per = TL._call(args, d, clean)
    TL._check_rows(f"clip {name}", d_np, [[b] for b in range(B)], th, pm, per, 0.05)
    lr_on, g_on = masking_loss(d, clean, args, grad=True)
    lr_off, _ = masking_loss(d, clean, _args())
    torch.cuda.synchronize()
    assert torch.equal(lr_on, per["rows"]) and torch.equal(g_on, -per["grad"])
    assert bool((lr_on <= lr_off).all()) and bool((lr_on < lr_off).any())          # A' >= A: every hinge term can only shrink


def test_burst_clip_gains_room_after_the_burst():
    x_np = _clean("burst")
    L = x_np.shape[1]
    d_np = _noise(1, L, 1e-2)
    clean, d = _dev(x_np), torch.from_numpy(d_np).cuda()
    out = {}
    for key, times in (("off", None), ("on", TIMES[0])):
        args = _args(times)
        out[key] = _proj_rows(runtime.get_proj(args, "cuda", 1, L), runtime.params_of(args), d, clean)
    torch.cuda.synchronize()
    on, off = out["on"][0].double().cpu().numpy(), out["off"][0].double().cpu().numpy()
    e_on, e_off = float((on[8192:13000] ** 2).sum()), float((off[8192:13000] ** 2).sum())
    print(f"energy in samples 8192..13000: off {e_off:.4e}, on {e_on:.4e}")
    assert e_on > e_off
    assert np.abs(on[:3000] - off[:3000]).max() <= 1e-6


@pytest.mark.parametrize("kind", ["pgd", "clip"])
def test_steppers_replay_as_they_run_and_loss_falls(kind):
    B, L, alpha = 2, 16000, 5e-6
    clean = _dev(_clean("3x16000")[:B])
    nrows = B if kind == "clip" else 1
    d0 = torch.from_numpy(_noise(B, L, 3e-2)[:nrows]).cuda()
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    first = {}
    for key, times in (("off", None), ("on", TIMES[0])):
        args = _args(times, masking_loss_alpha=alpha, lr=1e-3)
        labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
        make = lambda: PgdStepper(m, args, L) if nrows == 1 else ClipStepper(m, args, L)
        st, p = make(), d0.clone()
        for i in range(3):
            r = st.step(p, clean, labels)
            if i == 0:
                first[key] = r["masking_loss"].clone()
        torch.cuda.synchronize()
        eager = (p.clone(), st.grad.clone(), r["masking_loss"].clone())
        st, q = make(), d0.clone()
        g, r = st.capture(q, clean, labels)
        q.copy_(d0)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(q, eager[0]) and torch.equal(st.grad, eager[1]) and torch.equal(r["masking_loss"], eager[2]), (kind, key)
        first[key + "_p"] = eager[0]
    assert bool((first["on"] <= first["off"]).all()) and bool((first["off"] > 0).all())          # l_b of the same delta
    assert not torch.equal(first["on_p"], first["off_p"])                                         # the mode is in the step


def test_setter_refusals():
    lib = _lib.lib()
    pr = runtime.Proj("cuda", 1024, 256, 1024, 16000, 1, 4096)
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    call = lambda h, post, pre: lib.paa_proj_set_masking_spread(h, len(post), post.ctypes.data if len(post) else None,
                                                                len(pre), pre.ctypes.data if len(pre) else None)
    ok, none = f32(4.8 * np.arange(1, 20)), f32([])
    bad = {"33 entries": f32(np.arange(1, 34)), "decreasing": f32([4.8, 9.6, 9.5]), "negative": f32([-1.0, 2.0]), "zero": f32([0.0, 1.0]),
           "nan": f32([1.0, np.nan]), "inf": f32([1.0, np.inf])}
    for why, tab in bad.items():
        assert call(pr.h, tab, none) == _lib.PAA_ERR_ARG, why
        assert call(pr.h, ok, tab) == _lib.PAA_ERR_ARG, why
    assert lib.paa_proj_set_masking_spread(pr.h, -1, None, 0, None) == _lib.PAA_ERR_ARG
    assert lib.paa_proj_set_masking_spread(pr.h, 2, None, 0, None) == _lib.PAA_ERR_ARG             # a null table with n > 0
    assert call(pr.h, f32(np.arange(1, 33)), f32([3.0, 3.0])) == _lib.PAA_OK                      # 32 entries; equal neighbours
    assert call(pr.h, none, none) == _lib.PAA_OK
    odd = runtime.Proj("cuda", 512, 128, 512, 16000, 1, 4096)                                      # a non-default geometry
    assert call(odd.h, ok, none) == _lib.PAA_ERR_ARG and call(odd.h, none, none) == _lib.PAA_ERR_ARG
    # a refused call leaves the handle as it was: still off, the parent's bits
    x = _dev(_clean("2x4096")[:1])
    th = torch.empty(1, 17, F, device="cuda")
    assert call(pr.h, f32([5.0, 4.0]), none) == _lib.PAA_ERR_ARG
    _threshold_into(pr, x, th)
    torch.cuda.synchronize()
    assert torch.equal(th, _theta_off("2x4096")[0][:1])
    with pytest.raises(ValueError, match="masking_post_ms"):                                        # the Python layer refuses before the library
        runtime.get_proj(_args((1000.0, 0.0)), "cuda", 1, 4096)


# ------------------------------------------------------------------------------------------------ runners
def _walk(root, name):
    return [os.path.join(d, name) for d, _, fs in os.walk(root) if name in fs]


def _run(module, tmp_path, tag, extra):
    logs = str(tmp_path / tag)
    common = ["--arch", "tiny", "--device", "cuda", "--audio_seconds", "0.5", "--batch_size", "2", "--steps_per_epoch", "1", "--silent",
              "--optimizer_type", "pgd", "--dtype", "fp32", "--logs_dir", logs, "--norm_type", "masking", "--masking_loss_alpha", "1e-6",
              "--masking_post_ms", "200", "--masking_pre_ms", "20"]
    assert subprocess.run([sys.executable, "-m", module] + common + extra, cwd=ROOT, timeout=600).returncode == 0
    return logs


def test_attack_clips_names_the_run_and_writes_the_keys(tmp_path):
    extra = ["--small_data", "--pgd_steps", "3", "--num_items_to_inspect", "0"]
    found = [_walk(_run("paa_amd.attack_clips", tmp_path, tag, extra), "clip_results.json") for tag in ("a", "b")]
    assert all(len(f) == 1 for f in found)
    assert "_ml1e-06_mt200-20_" in found[0][0]
    res = json.load(open(found[0][0]))
    assert res["masking_post_ms"] == 200.0 and res["masking_pre_ms"] == 20.0
    assert res["clips"] and all(np.isfinite(c["final_ctc"]) and np.isfinite(c["final_masking_loss"]) for c in res["clips"])
    assert open(found[0][0], "rb").read() == open(found[1][0], "rb").read()
    assert os.path.relpath(found[0][0], str(tmp_path / "a")) == os.path.relpath(found[1][0], str(tmp_path / "b"))


def test_run_attack_names_the_run_and_writes_the_keys(tmp_path):
    extra = ["--num_epochs", "1"]
    found = [_walk(_run("paa_amd.run_attack", tmp_path, tag, extra), "results.json") for tag in ("a", "b")]
    assert all(len(f) == 1 for f in found)
    assert "_ml1e-06_mt200-20_" in found[0][0]
    res = json.load(open(found[0][0]))
    assert res.get("finished_training") == 1.0
    assert res["masking_post_ms"] == 200.0 and res["masking_pre_ms"] == 20.0 and res["masking_loss_alpha"] == 1e-6
    assert open(found[0][0], "rb").read() == open(found[1][0], "rb").read()
    assert os.path.relpath(found[0][0], str(tmp_path / "a")) == os.path.relpath(found[1][0], str(tmp_path / "b"))


def test_runners_refuse_a_time_without_a_consumer(tmp_path):
    from paa_amd import attack_clips, run_attack
    from paa_amd.training_utils import parser
    flags = ["--norm_type", "linf", "--masking_post_ms", "200", "--logs_dir", str(tmp_path)]
    with pytest.raises(ValueError, match="masking_post_ms"):
        run_attack.main(parser.create_arg_parser().parse_args(flags))
    with pytest.raises(ValueError, match="masking_post_ms"):
        attack_clips.main(attack_clips.create_arg_parser().parse_args(flags))
    with pytest.raises(ValueError, match=r"\(10, 330\]"):
        attack_clips.main(attack_clips.create_arg_parser().parse_args(["--norm_type", "masking", "--masking_pre_ms", "5"]))
