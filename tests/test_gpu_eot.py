"""-m gpu: per-clip perturbations through the playback chain — paa_eot_rows / paa_eot_reduce / paa_eot_vote
against tests/eot_ref.py between guard blocks, the step with the chain on against the oracle, the identity chain against the plain
per-clip step, the launch order, the draws inside captured graphs, the identity of a clip's draws across batches, the bound search
on the voted counters, and the runner.

Bounds.  paa_eot_rows is one f32 add and one f32 multiply, paa_eot_reduce a sum of exact products rounded once: both are compared
bit for bit.  The drifted / wet rows of the step are held to chan_ref.bound / rir_ref.bound (derived there) plus the bound of the
link before them carried through the rooms.  The step bounds are those of test_gpu_rir.test_reverberant_step_vs_oracle, the same
composition."""
import json
import os

import numpy as np
import pytest
import torch

import chan_ref as CR
import eot_ref as ER
import place_ref as PR
import rir_ref as RR
import search_ref as SR
from gpu_util import record_launches, rel_err
from oracle import pgd as opgd, projections as OP, wav2vec2 as OW
from oracle.gen_cases import PGD_TEXTS, cli_to_args
from paa_amd import _lib, arch as A, runtime, synth
from paa_amd.core import loss_helpers
from paa_amd.model import PaaModel
from paa_amd.training_utils import build, rir
from paa_amd.training_utils.clip_attack import ClipStepper, SearchConfig

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF          # a NaN pattern no kernel writes
ROWS_CASES = [(1, 1, 1), (1, 5, 257), (3, 4, 1000), (2, 3, 4099), (4, 8, 8000)]
OTHER = "zq zq zq"


@pytest.fixture(scope="module", autouse=True)
def _fresh_projection_contexts():
    yield
    torch.cuda.synchronize()
    runtime._PROJ.clear()


class Guarded:
    """A 4-byte device tensor between two guard blocks of a sentinel pattern, ``offset`` floats past a 16-byte boundary; the tensor
    itself starts as the sentinel too."""

    def __init__(self, shape, dtype=torch.float32, offset=0, fill=None):
        shape = tuple(int(s) for s in shape)
        self.n, self.g, self.o = int(np.prod(shape)), 256, int(offset)
        self.full = torch.full((self.n + 2 * self.g + self.o,), SENT, dtype=torch.int32, device="cuda")
        self.t = self.full[self.g + self.o:self.g + self.o + self.n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 4 * (self.o % 4)
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)).view(shape))

    @property
    def ptr(self):
        return _lib.ptr(self.t)

    def check(self):
        lo, hi = self.g + self.o, self.g + self.o + self.n
        assert bool((self.full[:lo] == SENT).all()) and bool((self.full[hi:] == SENT).all()), "guard overwritten"

    def untouched(self):
        return bool((self.full[self.g + self.o:self.g + self.o + self.n] == SENT).all())


def _normal(shape, tag, scale=1.0):
    n = int(np.prod(shape))
    return (synth.normal(synth.key_of(f"eot_{tag}_{n}", 5), n) * scale).astype(np.float32).reshape(shape)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- 1. paa_eot_rows / paa_eot_reduce --------------------------------------------------------------------------------------
def _rows_and_reduce(B, G, L, with_gain, with_clean, offset):
    lib, st, R = _lib.lib(), _lib.stream_ptr(), B * G
    x, d, grows = _normal((B, L), "x"), _normal((B, L), "d", 1e-2), _normal((R, L), "g")
    a = np.exp2(_normal((R,), "a", 0.5)).astype(np.float32)
    clean = Guarded((B, L), offset=offset, fill=x) if with_clean else None
    delta, gain = Guarded((B, L), offset=offset, fill=d), Guarded((R,), offset=offset, fill=a) if with_gain else None
    rows, crow = Guarded((R, L), offset=offset), Guarded((R, L), offset=offset) if with_clean else None
    ptr = lambda g: None if g is None else g.ptr
    for _ in range(2):                                           # two calls: the same bits
        _lib.check(lib.paa_eot_rows(ptr(clean), delta.ptr, ptr(gain), rows.ptr, ptr(crow), B, G, L, st))
        torch.cuda.synchronize()
        want = ER.rows32(x if with_clean else None, d, a if with_gain else None, G)
        assert np.array_equal(_bits(rows.t.cpu().numpy()), _bits(want)), (B, G, L, with_gain, with_clean, offset)
        if with_clean:
            assert np.array_equal(_bits(crow.t.cpu().numpy()), _bits(ER.clean_rows(x, G)))
    src, grad = Guarded((R, L), offset=offset, fill=grows), Guarded((B, L), offset=offset)
    _lib.check(lib.paa_eot_reduce(src.ptr, ptr(gain), grad.ptr, B, G, L, st))
    torch.cuda.synchronize()
    want = ER.reduce64(grows, a if with_gain else None, G)
    assert np.array_equal(_bits(grad.t.cpu().numpy()), _bits(want)), (B, G, L, with_gain, offset)
    for g in (clean, delta, gain, rows, crow, src, grad):
        if g is not None:
            g.check()
    assert np.array_equal(_bits(delta.t.cpu().numpy()), _bits(d)) and np.array_equal(_bits(src.t.cpu().numpy()), _bits(grows))


@pytest.mark.parametrize("B,G,L", ROWS_CASES)
def test_rows_and_reduce_bit_equal_to_the_reference(B, G, L):
    for with_gain in (True, False):
        for with_clean in (True, False):
            _rows_and_reduce(B, G, L, with_gain, with_clean, 0)
    _rows_and_reduce(B, G, L, True, True, 1)                    # every pointer one float past a 16-byte boundary


@pytest.mark.parametrize("B,G,L", ROWS_CASES)
def test_reduce_of_one_clip_is_place_reduce(B, G, L):
    lib, st = _lib.lib(), _lib.stream_ptr()
    grows, a = _normal((G, L), "pg"), np.exp2(_normal((G,), "pa", 0.5)).astype(np.float32)
    src, gain = Guarded((G, L), fill=grows), Guarded((G,), fill=a)
    zero = torch.zeros(G, dtype=torch.int32, device="cuda")
    mine, theirs = Guarded((1, L)), Guarded((L,))
    _lib.check(lib.paa_eot_reduce(src.ptr, gain.ptr, mine.ptr, 1, G, L, st))
    _lib.check(lib.paa_place_reduce(src.ptr, _lib.ptr(zero), gain.ptr, theirs.ptr, G, L, L, st))
    torch.cuda.synchronize()
    mine.check(), theirs.check()
    assert torch.equal(mine.t.view(torch.int32).view(-1), theirs.t.view(torch.int32))


def test_refusals_leave_outputs_alone():
    lib, st, ARG = _lib.lib(), _lib.stream_ptr(), _lib.PAA_ERR_ARG
    B, G, L = 2, 3, 100
    x, gain = torch.zeros(B * G, L, device="cuda"), torch.ones(B * G, device="cuda")
    cnt = torch.zeros(B * G, 3, dtype=torch.int32, device="cuda")
    rows, crow, grad, out = Guarded((B * G, L)), Guarded((B * G, L)), Guarded((B, L)), Guarded((B, 3), torch.int32)
    px, pg = _lib.ptr(x), _lib.ptr(gain)
    for B_, G_, L_ in ((0, G, L), (B, 0, L), (B, G, 0), (1 << 16, 1 << 15, L)):
        assert lib.paa_eot_rows(px, px, pg, rows.ptr, crow.ptr, B_, G_, L_, st) == ARG
        assert lib.paa_eot_reduce(px, pg, grad.ptr, B_, G_, L_, st) == ARG
        if L_:
            assert lib.paa_eot_vote(_lib.ptr(cnt), B_, G_, 0, out.ptr, st) == ARG
    assert lib.paa_eot_rows(px, None, pg, rows.ptr, crow.ptr, B, G, L, st) == ARG
    assert lib.paa_eot_rows(None, px, pg, rows.ptr, crow.ptr, B, G, L, st) == ARG          # a per-row clean copy without the clean batch
    assert lib.paa_eot_reduce(None, pg, grad.ptr, B, G, L, st) == ARG
    assert lib.paa_eot_vote(None, B, G, 1, out.ptr, st) == ARG
    with pytest.raises(_lib.PaaError, match="null"):
        _lib.check(lib.paa_eot_rows(px, px, pg, None, None, B, G, L, st))
    torch.cuda.synchronize()
    for g in (rows, crow, grad, out):
        g.check()
        assert g.untouched()


# ---- 2. paa_eot_vote -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 7])
def test_vote_is_exact(G):
    rng = np.random.default_rng(G)
    for B in (1, 5, 300):                                        # 300: past one block
        c = np.stack([rng.integers(0, 4, B * G), rng.integers(1, 6, B * G), rng.integers(0, 9, B * G)], axis=1).astype(np.int32)
        if G > 1 and B == 300:
            assert any(len(set(c[b * G:(b + 1) * G, 0])) < G for b in range(B))              # ties are in
        rows = torch.from_numpy(c).cuda()
        for targeted in (0, 1):
            out = Guarded((B, 3), torch.int32)
            _lib.check(_lib.lib().paa_eot_vote(_lib.ptr(rows), B, G, targeted, out.ptr, _lib.stream_ptr()))
            torch.cuda.synchronize()
            out.check()
            assert out.t.cpu().tolist() == ER.vote(c, G, bool(targeted)).tolist(), (B, G, targeted)


# ---- 3. the step against the oracle ----------------------------------------------------------------------------------------
STEP_N, STEP_K = 3, 600


def _chain_args(norm="linf", extra=(), **kw):
    args = cli_to_args(norm, list(extra))
    args.device, args.sr, args.seed = "cuda", 16000, 5
    for k, v in kw.items():
        setattr(args, k, v)
    return args


@pytest.mark.parametrize("variant", ["group", "layer"])
def test_eot_step_vs_oracle(variant):
    a = A.tiny("group", False) if variant == "group" else A.tiny("layer", True)
    B, G, L = 2, 3, 16000
    R = B * G
    args = _chain_args(place_gain_db=6.0, rir_bank="synthetic", rir_count=STEP_N, rir_taps=STEP_K, drift_ppm=90000.0)
    gains = np.array([0.7, 1.3, 1.0, 0.9, 1.15, 0.8], dtype=np.float32)
    rooms, rq = [1, 2, 0, 2, 2, 1], [CR.rq_of(r) for r in (0.97, 1.0 + 3e-3, 1.0, 1.05, 0.999, 1.02)]
    bank_np = rir.bank_of(args)
    sdn = A.rule_weights(a)
    sd = OW.to_torch(sdn)
    clean = torch.from_numpy(synth.clean_audio(B, L))
    d0 = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * 1e-3)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    lab_rows = labels.repeat_interleave(G, dim=0)
    spl = OP.spl_thresh_tensor(args)
    m = PaaModel(a, sdn, R, L, "fp32")
    st = ClipStepper(m, args, L, None, build.init_phon_threshold_tensor(args), eot_draws=G)
    assert st.G == G and st.max_batch == B and st.chain.placer.rows.shape == (R, L) and st.chain.clean_rows is None
    st.set_gains(gains), st.set_rooms(rooms), st.set_channel(rq)
    d = d0.cuda()
    with record_launches() as names:
        r = st.step(d, clean.cuda(), labels)
    torch.cuda.synchronize()
    assert not any(n.endswith("_draw") for n in names)           # pinned: nothing drawn
    g = st.grad.cpu().numpy()
    assert g.shape == (B, L) and r["grad_rows"].shape == (R, L)
    # the chain rows -> drift -> rooms in numpy float64, every link held to its own derived bound
    rows0 = ER.rows32(clean.numpy(), d0.numpy(), gains, G)
    assert np.array_equal(_bits(st.chain.placer.rows.cpu().numpy()), _bits(rows0))
    dry64 = CR.apply64(rq, rows0)
    b_dry = CR.bound(rq, rows0)
    dry_dev = st.chain.chan.rows.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(dry_dev - dry64) <= b_dry), float((np.abs(dry_dev - dry64) / b_dry).max())
    wet64 = RR.apply64(bank_np, rooms, dry64)
    wet_dev = st.chain.reverb.rows.cpu().numpy().astype(np.float64)
    b_wet = RR.bound(bank_np, rooms, dry_dev) + RR.apply64(np.abs(bank_np), rooms, b_dry)        # the rooms' own + the drift's, carried
    assert np.all(np.abs(wet_dev - wet64) <= b_wet), float((np.abs(wet_dev - wet64) / b_wet).max())
    ref = opgd.pgd_step(sd, a, args, torch.zeros(R, L), lab_rows, torch.from_numpy(wet64.astype(np.float32)), spl)
    grows = CR.adjoint64(rq, RR.adjoint64(bank_np, rooms, ref["grad"].numpy().astype(np.float64)))
    gref = ER.reduce64(grows.astype(np.float32), gains, G).astype(np.float64)
    e_g = max(rel_err(g[b], gref[b]) for b in range(B))
    flips = float((np.sign(g) != np.sign(gref)).mean())
    e_loss = abs(float(r["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    with torch.no_grad():
        pexp = torch.cat([OP.perturbation_constraint(d0[b:b + 1] + args.lr * torch.from_numpy(g[b:b + 1]).sign(), None, args, spl)
                          for b in range(B)])
    e_p = rel_err(d.cpu().numpy(), pexp.numpy())
    print(f"eot step {variant}: grad rel {e_g:.2e} flips {flips:.2e} loss rel {e_loss:.2e} p' rel {e_p:.2e}")
    assert e_g < 5e-3 and flips < 5e-3 and e_loss < 2e-4 and e_p < 5e-5, (e_g, flips, e_loss, e_p)


# ---- 4. the identity chain -------------------------------------------------------------------------------------------------
def _tiny_case(R, L, args):
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), R, L, "fp32")
    return m


def _start(B, L, scale=1e-3):
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    d0 = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * scale).cuda()
    return clean, d0


def test_identity_chain_is_the_plain_step(tmp_path):
    B, L = 2, 8000
    path = str(tmp_path / "one.npy")
    np.save(path, np.ones((1, 1), dtype=np.float32))
    args = _chain_args(extra=["--linf_size", "0.01"], rir_bank=path)
    plain_args = _chain_args(extra=["--linf_size", "0.01"])
    m = _tiny_case(B, L, args)
    clean, d0 = _start(B, L)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    eot, plain = ClipStepper(m, args, L, eot_draws=1), ClipStepper(m, plain_args, L)
    assert eot.chain.reverb.K == 1 and eot.chain.chan is None and eot.chain.placer.explicit
    de, dp = d0.clone(), d0.clone()
    for k in range(3):
        eot.step(de, clean, labels)
        plain.step(dp, clean, labels)
        torch.cuda.synchronize()
        assert torch.equal(de, dp), k
        assert torch.equal(eot.grad, plain.grad), k
    assert not torch.equal(de, d0)


# ---- 5. composition and order ----------------------------------------------------------------------------------------------
ALL = dict(place_gain_db=6.0, rir_bank="synthetic", rir_count=4, rir_taps=200, drift_ppm=20000.0, noise_snr_db=[20.0, 30.0])


def test_launch_order_and_gradient_by_hand():
    B, G, L = 2, 2, 8000
    R = B * G
    args = _chain_args(extra=["--linf_size", "0.01"], **ALL)
    m = _tiny_case(R, L, args)
    clean, d0 = _start(B, L)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    st = ClipStepper(m, args, L, eot_draws=G)
    d = d0.clone()
    seq = ["paa_place_draw", "paa_eot_rows", "paa_chan_draw", "paa_drift_apply", "paa_rir_draw", "paa_rir_apply", "paa_noise_add",
           "paa_model_fwd_bwd_rows", "paa_rir_apply", "paa_drift_apply", "paa_eot_reduce", "paa_sign_step", "paa_project_rows"]
    for _ in range(2):
        with record_launches() as names:
            st.step(d, clean, labels)
        assert names == seq, names                               # once per step, in the chain's order
    torch.cuda.synchronize()
    ch, lib, s = st.chain, _lib.lib(), _lib.stream_ptr()
    t1, t2, out = torch.empty(R, L, device="cuda"), torch.empty(R, L, device="cuda"), Guarded((B, L))
    _lib.check(lib.paa_rir_apply(_lib.ptr(ch.reverb.bank), ch.reverb.N, ch.reverb.K, _lib.ptr(ch.reverb.index),
                                 _lib.ptr(ch.placer.grad_rows), _lib.ptr(t1), R, L, 1, s))
    _lib.check(lib.paa_drift_apply(_lib.ptr(ch.chan.rq), _lib.ptr(t1), _lib.ptr(t2), R, L, 1, s))
    _lib.check(lib.paa_eot_reduce(_lib.ptr(t2), _lib.ptr(ch.placer.gain), out.ptr, B, G, L, s))
    torch.cuda.synchronize()
    out.check()
    assert torch.equal(out.t, st.grad) and float(st.grad.abs().max()) > 0
    assert torch.equal(ch.clean_rows[:R], clean.repeat_interleave(G, dim=0))          # the noise's level reference, per row
    # with the bound search: the vote sits between the counters and the search, the adjoints behind it
    cfg = SearchConfig(0.8, 0.01, 500, False)
    ss = ClipStepper(m, args, L, device_wer=True, search=cfg, eot_draws=G)
    ss.set_refs(loss_helpers.encode_refs([OTHER] * B))
    ss.search_reset(B)
    with record_launches() as names:
        ss.step(d0.clone(), clean, labels)
    order = ["paa_noise_add", "paa_model_fwd_bwd_rows", "paa_wer_counts", "paa_eot_vote", "paa_clip_search", "paa_rir_apply",
             "paa_eot_reduce", "paa_sign_step", "paa_project_rows_scaled"]
    at = [len(names) - 1 - names[::-1].index(n) for n in order]
    assert at == sorted(at) and names.count("paa_eot_vote") == 1 and "paa_project_rows" not in names, names


# ---- 6. graphs -------------------------------------------------------------------------------------------------------------
def test_capture_and_replays_equal_eager_steps_and_draw_anew():
    B, G, L, c0, base = 2, 2, 8000, 4, 10
    R = B * G
    args = _chain_args(extra=["--linf_size", "0.01"], **ALL)
    m = _tiny_case(R, L, args)
    clean, d0 = _start(B, L)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    st_g, st_e = ClipStepper(m, args, L, eot_draws=G), ClipStepper(m, args, L, eot_draws=G)
    for st in (st_g, st_e):
        st.set_eot_clip(base // G)
        st.set_eot_step(c0)
    assert st_g.chain.clip_base == base
    d_g, d_e = d0.clone(), d0.clone()
    g, _ = st_g.capture(d_g, clean, labels)
    torch.cuda.synchronize()
    counters = st_g.chain.counters()
    assert len(counters) == 4 and [int(c.item()) for c in counters] == [c0] * 4          # capture() hands every counter back ...
    assert torch.equal(d_g, d0)                                                              # ... and delta
    D, heard = CR.drift_q32(20000.0), []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        ch = st_g.chain
        a_ref = np.array([PR.draw_gain64(5, c0 + k, base + r, 0, 6.0) for r in range(R)])
        assert np.all(np.abs(ch.placer.gain.cpu().numpy() - a_ref) <= 1e-6 * a_ref), k
        assert ch.placer.shift.cpu().tolist() == [0] * R
        assert ch.reverb.index.cpu().tolist() == RR.draw(5, c0 + k, base, R, 0, 4).tolist(), k
        want_rq, want_snr = CR.draw(5, c0 + k, base, R, 0, D, 20.0, 30.0)
        assert ch.chan.rq.cpu().tolist() == want_rq, k
        assert np.allclose(ch.chan.snr_db.cpu().numpy(), want_snr, rtol=0, atol=4e-6)
        assert [int(c.item()) for c in counters] == [c0 + k + 1] * 4, k
        st_e.step(d_e, clean, labels)
        torch.cuda.synchronize()
        assert torch.equal(st_e.chain.reverb.rows, ch.reverb.rows) and torch.equal(d_e, d_g), k
        heard.append(ch.reverb.rows.clone())
    assert not torch.equal(heard[0], heard[1]) and not torch.equal(d_g, d0)


def test_noise_is_fresh_under_pinned_gains_and_follows_the_clean_level():
    """Gain and noise only, the gains pinned and lr = 0: delta stays, so what a replay hears differs from the last one by the
    noise alone — sigma_r z with sigma from the clean CLIP's level (clean_rows), z of row id clip_base + r at the step's counter."""
    B, G, L, base = 2, 2, 4000, 6
    R = B * G
    args = _chain_args(extra=["--linf_size", "0.01"], place_gain_db=6.0, noise_snr_db=[20.0, 30.0], lr=0.0)
    m = _tiny_case(R, L, args)
    clean, d0 = _start(B, L)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    st = ClipStepper(m, args, L, eot_draws=G)
    gains, snrs = np.array([0.8, 1.2, 1.0, 0.9], dtype=np.float32), np.array([30.0, 24.0, 20.0, 27.0], dtype=np.float32)
    st.set_gains(gains), st.set_channel([1.0] * R, snrs), st.set_eot_clip(base // G)
    assert float(d0.abs().max()) < 0.01                          # inside the bound: the projection leaves delta alone too
    d = d0.clone()
    g, _ = st.capture(d, clean, labels)
    dry = ER.rows32(clean.cpu().numpy(), d0.cpu().numpy(), gains, G).astype(np.float64)
    sig = CR.sigma64(ER.clean_rows(clean.cpu().numpy(), G), snrs)
    seen = []
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(d, d0), k
        z = st.chain.placer.rows.cpu().numpy().astype(np.float64) - dry          # the noise lands on the last buffer, in place
        want = np.stack([sig[r] * CR.noise64(5, k, base + r, 0, L) for r in range(R)])
        # the f32 add rounds at the level of the row, the noise itself follows the reference to 1e-5 of its peak
        assert np.abs(z - want).max() <= 1e-5 * np.abs(want).max() + 2.0 ** -23 * np.abs(dry).max(), k
        seen.append(z)
    assert int(st.chain.chan.noise_counter.item()) == 2 and int(st.chain.chan.counter.item()) == 0
    assert np.abs(seen[0] - seen[1]).max() > 0.1 * np.abs(seen[0]).max()


# ---- 7. the identity of a clip's draws -------------------------------------------------------------------------------------
def test_a_clips_draws_do_not_depend_on_its_batch():
    G, L = 3, 4000
    args = _chain_args(extra=["--linf_size", "0.01"], **ALL)
    clean4, d4 = _start(4, L)
    texts = [PGD_TEXTS[b % len(PGD_TEXTS)] for b in range(4)]
    m4, m2 = _tiny_case(4 * G, L, args), _tiny_case(2 * G, L, args)
    s4, s2 = ClipStepper(m4, args, L, eot_draws=G), ClipStepper(m2, args, L, eot_draws=G)
    s4.set_eot_clip(0), s2.set_eot_clip(2)                       # the 4-clip batch from index 0, the 2-clip batch from index 2
    da, db = d4.clone(), d4[2:].clone()
    for k in range(3):
        s4.step(da, clean4, opgd.make_labels(texts, args, 4))
        s2.step(db, clean4[2:].contiguous(), opgd.make_labels(texts[2:], args, 2))
        torch.cuda.synchronize()
        for name in ("placer.gain", "reverb.index", "chan.rq", "chan.snr_db"):
            site, buf = name.split(".")
            big, small = getattr(getattr(s4.chain, site), buf), getattr(getattr(s2.chain, site), buf)
            assert torch.equal(big[2 * G:3 * G], small[:G]), (k, name)
        if k == 0:          # the same delta entered: what clip 2 hears is the same, noise included
            assert torch.equal(s4.chain.reverb.rows[2 * G:3 * G], s2.chain.reverb.rows[:G])
    assert [int(c.item()) for c in s4.chain.counters()] == [3] * 4


# ---- 8. the bound search on the voted counters -----------------------------------------------------------------------------
@pytest.mark.parametrize("targeted", [False, True])
def test_bound_search_follows_the_voted_counters(targeted):
    B, G, L, steps = 2, 2, 16000, 4
    R = B * G
    mode = ["--attack_mode", "targeted", "--target", "delete", "--target_reps", "1"] if targeted else []
    args = _chain_args(extra=["--linf_size", "0.01", *mode], **ALL)
    m = _tiny_case(R, L, args)
    clean, d0 = _start(B, L)
    labels = opgd.make_labels(PGD_TEXTS[:B], args, B)
    cfg = SearchConfig(0.8, 0.01, 500, targeted)
    # clip 1 is judged against what the model writes for its start, heard directly: its draws fail until the channel or the attack
    # changes a word
    r0 = m.fwd_bwd(clean, d0, labels, +1, want_grad=False)
    torch.cuda.synchronize()
    ids = loss_helpers.argmax_ids(r0["logits"], None, int(m.arch.pad_token_id))
    own = [t.strip().lower() for t in loss_helpers.greedy_decode_ids(ids.cpu().tolist())][1]
    refs = [OTHER, OTHER if targeted or not own.split() else own]
    st = ClipStepper(m, args, L, device_wer=True, search=cfg, eot_draws=G)
    st.set_refs(loss_helpers.encode_refs(refs))
    st.search_reset(B)
    scale, best = np.ones(B, dtype=np.float32), np.zeros((B, L), dtype=np.float32)
    best_scale, best_step, step_no = np.ones(B, dtype=np.float32), np.full(B, -1, dtype=np.int32), 0
    d, hist = d0.clone(), []
    for k in range(steps):
        entered = d.cpu().numpy()
        st.step(d, clean, labels)
        torch.cuda.synchronize()
        rows = st.wer_rows[:R].cpu().numpy()
        voted = st.wer_clips[:B].cpu().numpy()
        assert np.array_equal(voted, ER.vote(rows, G, targeted)), (k, rows, voted)
        assert np.array_equal(rows[:, 1], np.repeat([len(r.split()) for r in refs], G))          # the references, repeated per row
        hist.append(SR.success(voted, targeted, cfg.wer_milli))
        scale, best, best_scale, best_step, step_no = SR.clip_search(entered, voted, targeted, cfg.wer_milli, cfg.shrink, cfg.floor_scale,
                                                                     scale, best, best_scale, best_step, step_no)
        assert np.array_equal(st.scale[:B].cpu().numpy(), scale) and np.array_equal(st.best_step[:B].cpu().numpy(), best_step), k
        assert int(st.search_step.item()) == step_no
        found = best_step >= 0
        assert np.array_equal(st.best_scale[:B].cpu().numpy()[found], best_scale[found])
        assert np.array_equal(st.best[:B].cpu().numpy()[found], best[found])
        assert float(d.abs().max()) <= 0.01 * float(scale.max()) * (1 + 1e-6)
    print(f"success per step and clip\n{np.array(hist).astype(int)}\nscales {scale}")
    if targeted:          # the target is never written: no draw succeeds, nothing is kept, no bound moves
        assert not np.array(hist).any() and (best_step == -1).all() and (scale == 1).all()
    else:
        assert np.array(hist)[:, 0].all(), "no word of clip 0's reference is ever written: every draw succeeds at every step"


# ---- 9. the runner ---------------------------------------------------------------------------------------------------------
def _run(tmp, name, extra):
    from paa_amd import attack_clips
    logs = str(tmp / name)
    args = attack_clips.create_arg_parser().parse_args(
        ["--arch", "tiny", "--device", "cuda", "--dtype", "fp32", "--audio_seconds", "0.5", "--batch_size", "4", "--steps_per_epoch", "2",
         "--small_data", "--silent", "--norm_type", "linf", "--linf_size", "0.01", "--num_items_to_inspect", "0", "--pgd_steps", "3",
         "--eot_draws", "2", "--rir_bank", "synthetic", "--rir_taps", "64", "--noise_snr_db", "20", "30", "--logs_dir", logs, *extra])
    assert attack_clips.main(args) == 0
    path = os.path.join(args.save_dir, "clip_results.json")
    return args, path, json.load(open(path))


def test_runner_records_and_repeats(tmp_path):
    args, path, res = _run(tmp_path, "a", ["--optimizer_type", "pgd"])
    assert "_rir64x64_noise20-30_eot2_" in os.path.basename(args.save_dir), args.save_dir
    assert res["eot_draws"] == 2 and res["eot_eval_draws"] == 2 and res["rir_taps"] == 64 and res["noise_snr_db"] == [20.0, 30.0]
    clips = res["clips"]
    assert len(clips) >= 2 and [c["index"] for c in clips] == list(range(len(clips)))
    for c in clips:
        assert c["eot_draws"] == 2 and c["eot_adv_wer"] >= 0 and c["eot_clean_wer"] >= 0 and 0 <= c["eot_success"] <= 1
        assert c["eot_success"] in (0.0, 0.5, 1.0)                                   # a multiple of 1 / E
        assert 0 < c["linf"] <= 0.01 * (1 + 1e-6) and np.isfinite(c["final_ctc"])     # the norms bound delta itself
    for k in ("eot_adv_wer", "eot_clean_wer", "eot_success"):
        assert res["summary"][k] == sum(c[k] for c in clips) / len(clips)
    _, path2, _ = _run(tmp_path, "b", ["--optimizer_type", "pgd"])
    assert open(path, "rb").read() == open(path2, "rb").read()                      # the same draws, the same bytes
    _, _, res5 = _run(tmp_path, "c", ["--optimizer_type", "pgd", "--eot_eval_draws", "5"])          # three passes of two
    assert all(c["eot_draws"] == 5 and c["eot_success"] in [h / 5 for h in range(6)] for c in res5["clips"])
    _, _, adam = _run(tmp_path, "d", ["--optimizer_type", "adam", "--lr", "1e-3"])
    assert all(np.isfinite(c["final_ctc"]) and c["eot_draws"] == 2 and c["linf"] > 0 for c in adam["clips"])
