"""-m gpu: paa_wer_counts / paa_stats_push against the host string path (greedy_decode_ids + wer_texts + wer_counts), their error
contract, and the device_wer mode of the steppers, train_epoch, evaluate and attack_clips against the unflagged runs."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
R_CAP = 2048          # 750 one-letter words (T = 1499, alternating) take 1500 entries
TEXTS = ["ab cd", "hello", "a b c", "xyz w"]


def _counts(ids, texts, r_cap=R_CAP, sums=True):
    """(B, T) ids + texts -> ((B, 3) counters, (2,) sums) from the kernel."""
    from paa_amd.core import loss_helpers as LH
    refs = LH.encode_refs(texts, r_cap)
    assert refs is not None                                       # every case is inside the caps: nothing falls back
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int16)).cuda()
    s = torch.full((2,), -1.0, device="cuda") if sums else None
    out = LH.wer_counts_device(d_ids, refs, LH.canon_table(None), sums=s)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if s is None else s.cpu().numpy()


def _groups(T):
    import wer_ref as W
    cs = [c for c in W.cases(seed=0, per_cell=4) if len(c[1]) == T]
    assert len(cs) == 24
    return cs


@pytest.mark.parametrize("T", [1, 2, 7, 49, 499, 1499])
def test_kernel_equals_host_string_path(T):
    import wer_ref as W
    cs = _groups(T)
    want = np.array([W.host_counts(ids, ref) for _, ids, ref in cs], dtype=np.int32)
    if T == 1499:
        assert want[:, 2].max() == 750                            # the largest hypothesis the kernel is sized for
    alone = np.zeros_like(want)
    for i, (_, ids, ref) in enumerate(cs):                        # B = 1
        got, s = _counts(ids[None], [ref])
        alone[i] = got[0]
        assert s.tolist() == [float(got[0, 0]), float(got[0, 1])]
    bad = [(cs[i][0], alone[i].tolist(), want[i].tolist()) for i in range(len(cs)) if (alone[i] != want[i]).any()]
    assert not bad, bad[:5]
    for B in (3, 32):
        pick = [(k + j) % len(cs) for k in range(0, len(cs), B) for j in range(B)] if B == 3 else [j % len(cs) for j in range(32)]
        for k in range(0, len(pick), B):
            sel = pick[k:k + B]
            ids = np.stack([cs[i][1] for i in sel])
            texts = [cs[i][2] for i in sel]
            got, s = _counts(ids, texts)
            assert (got == want[sel]).all(), (B, k)                # equal to the host path, and to the clip alone
            assert (got == alone[sel]).all()
            assert s.tolist() == [float(got[:, 0].sum()), float(got[:, 1].sum())]
            again, s2 = _counts(ids, texts)
            assert (again == got).all() and (s2 == s).all()        # two runs: identical output


def test_kernel_from_logits_with_ties_and_nans():
    """The logits entry (paa_argmax_ids then paa_wer_counts) against wer_texts + wer_counts on the same logits; ties and NaNs
    resolve as torch.argmax does because the ids are paa_argmax_ids' own."""
    from paa_amd.core import loss_helpers as LH
    g = torch.Generator().manual_seed(7)
    B, T, V = 5, 499, 32
    logits = torch.randn(B, T, V, generator=g)
    logits[:, ::7, :] = 0.0                                        # all-tie frames: first maximum (<pad>) wins
    logits[1, 5, 9] = float("nan")
    logits[2, ::3, 4] = 9.0                                        # many delimiters
    texts = ["the cat", "", "a b c d e f", "it's", "zz <unk> top"]
    d = logits.cuda()
    got = LH.wer_counts_device(d, LH.encode_refs(texts), LH.canon_table(None)).cpu().tolist()
    pred, ref = LH.wer_texts(d, texts, None)
    for b in range(B):
        e, w = LH.wer_counts([pred[b]], [ref[b]])
        assert got[b] == [e, w, len(pred[b].split())], b


def test_error_contract():
    from paa_amd import _lib
    from paa_amd.core import loss_helpers as LH
    L = _lib.lib()
    B, T = 2, 49
    ids = torch.zeros(B, T, dtype=torch.int16, device="cuda")
    canon = LH.canon_table(None).cuda()
    out = torch.zeros(B, 3, dtype=torch.int32, device="cuda")
    big = torch.full((B, 8193), -1, dtype=torch.int32, device="cuda")
    ok = torch.full((B, 64), -1, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()

    def call(ids_, B_, T_, canon_, V_, refs_, R_, out_):
        return L.paa_wer_counts(_lib.ptr(ids_), B_, T_, _lib.ptr(canon_), V_, _lib.ptr(refs_), R_, _lib.ptr(out_), None, st)
    assert call(ids, B, T, canon, 32, ok, 64, out) == _lib.PAA_OK
    assert call(ids, B, T, canon, 32, big, 8193, out) == _lib.PAA_ERR_SIZE           # oversize R
    assert b"R_cap=8193" in L.paa_last_error()
    assert call(ids, B, 4097, canon, 32, ok, 64, out) == _lib.PAA_ERR_SIZE           # oversize T (nothing is launched)
    assert call(ids, B, 4096, canon, 32, big, 8192, out) == _lib.PAA_ERR_SIZE        # each inside its cap, together over the LDS
    assert b"LDS" in L.paa_last_error()
    assert call(None, B, T, canon, 32, ok, 64, out) == _lib.PAA_ERR_ARG
    assert call(ids, B, T, None, 32, ok, 64, out) == _lib.PAA_ERR_ARG
    assert call(ids, B, T, canon, 32, None, 64, out) == _lib.PAA_ERR_ARG
    assert call(ids, B, T, canon, 32, ok, 64, None) == _lib.PAA_ERR_ARG
    assert call(ids, 0, T, canon, 32, ok, 64, out) == _lib.PAA_ERR_ARG
    with pytest.raises(ValueError, match="R_cap=8193"):
        LH.wer_counts_device(ids, big, canon)
    stats = torch.zeros(8, device="cuda")
    log = torch.zeros(4, 8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.paa_stats_push(None, 8, _lib.ptr(log), _lib.ptr(cur), 4, st) == _lib.PAA_ERR_ARG
    assert L.paa_stats_push(_lib.ptr(stats), 8, _lib.ptr(log), None, 4, st) == _lib.PAA_ERR_ARG
    assert L.paa_stats_push(_lib.ptr(stats), 8, _lib.ptr(log), _lib.ptr(cur), 0, st) == _lib.PAA_ERR_ARG
    torch.cuda.synchronize()
    assert int(cur) == 0


def test_stats_push_appends_and_wraps():
    from paa_amd.training_utils.pgd import StatsLog
    log = StatsLog(torch.device("cuda"), cap=4, n=8)
    st = torch.zeros(8, device="cuda")
    for i in range(3):
        st.fill_(float(i + 1))
        log.push(st)
    rows = log.read()
    assert rows.tolist() == [[float(i + 1)] * 8 for i in range(3)]
    assert log.read().shape == (0, 8)                              # read() starts the log over
    g = torch.cuda.CUDAGraph()
    log.push(st)                                                   # warm-up outside the capture
    log.read()
    with torch.cuda.graph(g):
        log.push(st)
    for i in range(4):
        st.fill_(10.0 + i)
        g.replay()                                                 # the cursor advances on the device: one row per replay
    assert log.read().tolist() == [[10.0 + i] * 8 for i in range(4)]
    for _ in range(5):
        log.push(st)
    with pytest.raises(RuntimeError, match="overflow"):
        log.read()


# ------------------------------------------------------------------------------------------------ steppers
def _args(extra=()):
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args(["--arch", "tiny", "--dtype", "fp32", "--silent", "--optimizer_type", "pgd",
                                               "--norm_type", "snr", "--snr_db", "40", "--lr", "1e-3", *extra])
    a.device = "cuda"
    return a


def _host_counts_of(logits, texts):
    from paa_amd.core import loss_helpers as LH
    return [float(v) for v in LH.wer_counts(*LH.wer_texts(logits, texts, None))]


def _universal(arch, B, L, adam, device_wer, steps, collective=False, graph=False, dtype="fp32"):
    """``steps`` universal steps; returns p, per-step (loss, grad), the stepper's log rows and the host's counters per step."""
    from paa_amd import arch as A, synth
    from paa_amd.core import loss_helpers as LH
    from paa_amd.model import PaaModel
    from paa_amd.training_utils.pgd import PgdStepper
    args = _args(["--optimizer_type", "adam"] if adam else [])
    texts = TEXTS[:B]
    m = PaaModel(arch, A.rule_weights(arch), B, L, dtype)
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = LH.make_labels(texts, None, args, B)
    p = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L)
    opt = None
    if adam:
        p = torch.nn.Parameter(p)
        opt = torch.optim.Adam([p], lr=args.lr)
    st = PgdStepper(m, args, L, optimizer=opt, force_collective=collective, device_wer=device_wer)
    refs = LH.encode_refs(texts) if device_wer else None
    kw = {"refs": refs} if device_wer else {}
    trace, host = [], []
    if graph:
        p0 = p.detach().clone()
        logits = torch.empty(B, m.frames, arch.vocab_size, device="cuda")
        g, cap = st.capture(p.data, clean, labels, logits_out=logits, **kw)
        p.data.copy_(p0)
    for _ in range(steps):
        if graph:
            if device_wer:
                st.set_refs(refs)
            g.replay()
            lg = logits
        else:
            lg = st.step(p.data, clean, labels, **kw)["logits"]
        torch.cuda.synchronize()
        trace.append((float(st.stats[0]), st.grad.clone()))
        host.append(_host_counts_of(lg, texts))
    rows = st.read_log().tolist() if device_wer else None
    return p.detach().clone(), trace, rows, host, type(g).__name__ if graph else None


def _same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(x[0] == y[0] and torch.equal(x[1], y[1]) for x, y in zip(a[1], b[1]))


def _check_rows(rows, trace, host):
    assert len(rows) == len(trace)
    for row, (loss, _), hc in zip(rows, trace, host):
        assert row[0] == loss and row[3:5] == hc, (row, loss, hc)     # the logged counters are the host's of the SAME step


@pytest.mark.parametrize("adam", [False, True])
def test_universal_step_unchanged_and_counters_logged(adam):
    from paa_amd import arch as A
    off = _universal(A.tiny(), 3, 8000, adam, False, 4)
    on = _universal(A.tiny(), 3, 8000, adam, True, 4)
    assert _same(off, on)                                              # p, loss and gradient: the same bits
    _check_rows(on[2], on[1], on[3])
    assert on[3] == off[3] and any(h[1] > 0 for h in on[3])
    gr = _universal(A.tiny(), 3, 8000, adam, True, 4, graph=True)     # N replays: N rows, equal to N eager steps
    assert _same(gr, on) and gr[2] == on[2]


def test_universal_step_base_shape():
    from paa_amd import arch as A
    off = _universal(A.BASE, 2, 16000, False, False, 2)
    on = _universal(A.BASE, 2, 16000, False, True, 2)
    assert _same(off, on)
    _check_rows(on[2], on[1], on[3])


def _per_clip(adam, device_wer, steps, graph=False):
    from paa_amd import arch as A, synth
    from paa_amd.core import loss_helpers as LH
    from paa_amd.model import PaaModel
    from paa_amd.training_utils.clip_attack import ClipStepper
    a = A.tiny()
    B, L = 3, 8000
    args = _args(["--optimizer_type", "adam"] if adam else [])
    texts = TEXTS[:B]
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = LH.make_labels(texts, None, args, B)
    d = torch.from_numpy(np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32) * 1e-2).cuda()
    opt = None
    if adam:
        d = torch.nn.Parameter(d)
        opt = torch.optim.Adam([d], lr=args.lr)
    st = ClipStepper(m, args, L, optimizer=opt, device_wer=device_wer)
    refs = LH.encode_refs(texts) if device_wer else None
    kw = {"refs": refs} if device_wer else {}
    trace, host, clips = [], [], []
    if graph:
        d0 = d.detach().clone()
        logits = torch.empty(B, m.frames, a.vocab_size, device="cuda")
        g, cap = st.capture(d.data, clean, labels, logits_out=logits, **kw)
        d.data.copy_(d0)
    for _ in range(steps):
        if graph:
            g.replay()
            lg = logits
        else:
            lg = st.step(d.data, clean, labels, **kw)["logits"]
        torch.cuda.synchronize()
        trace.append((float(st.stats[0]), st.grad.clone()))
        host.append(_host_counts_of(lg, texts))
        if device_wer:
            pred, ref = LH.wer_texts(lg, texts, None)
            want = [[*LH.wer_counts([pred[b]], [ref[b]]), len(pred[b].split())] for b in range(B)]
            assert st.wer_rows[:B].cpu().tolist() == want              # the per-clip counters of the last step
    rows = st.read_log().tolist() if device_wer else None
    return d.detach().clone(), trace, rows, host


@pytest.mark.parametrize("adam", [False, True])
def test_per_clip_step_unchanged_and_counters_logged(adam):
    off = _per_clip(adam, False, 4)
    on = _per_clip(adam, True, 4)
    assert _same(off, on)
    _check_rows(on[2], on[1], on[3])
    gr = _per_clip(adam, True, 4, graph=True)
    assert _same(gr, on) and gr[2] == on[2]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_collective_step_one_rank_rccl():
    """force_collective=True over "nccl" in a fresh child interpreter (as tests/test_gpu_rccl.py does it): with device_wer the
    step's own all-reduce carries THIS step's counters; p, loss and gradient equal the unflagged collective stepper's bit for
    bit, eagerly and through the two-graph capture, PGD and Adam."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = json.loads([line for line in r.stdout.splitlines() if line.startswith("WER_RCCL ")][-1][len("WER_RCCL "):])
    print(d)
    assert d["backend"] == "nccl" and d["world"] == 1
    for k in ("pgd", "adam"):
        c = d[k]
        assert c["eager_same"] and c["graph_same"] and c["rows_eager_ok"] and c["rows_graph_ok"], (k, c)
        assert c["graph_type"] == "_SplitGraph" and c["n_rows"] == [3, 3]


def _rccl_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from paa_amd import arch as A
    out = {"backend": dist.get_backend(), "world": dist.get_world_size()}

    def rows_ok(run):
        return all(row[0] == loss and row[3:5] == hc for row, (loss, _), hc in zip(run[2], run[1], run[3]))
    for name, adam in (("pgd", False), ("adam", True)):
        off = _universal(A.tiny(), 3, 8000, adam, False, 3, collective=True)
        on = _universal(A.tiny(), 3, 8000, adam, True, 3, collective=True)
        gr = _universal(A.tiny(), 3, 8000, adam, True, 3, collective=True, graph=True)
        out[name] = {"eager_same": _same(off, on), "graph_same": _same(off, gr), "rows_eager_ok": rows_ok(on),
                     "rows_graph_ok": rows_ok(gr) and gr[2] == on[2], "graph_type": gr[4], "n_rows": [len(on[2]), len(gr[2])]}
    dist.destroy_process_group()
    print("WER_RCCL " + json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------ loops
def _loader(n, B, L):
    from paa_amd import synth
    texts = ["ab cd", "hello there", "a b c", "xyz w", "it's", "e", "the cat sat", "", "o n e"]
    return [(torch.from_numpy(synth.clean_audio(B, L, first_clip=i * B)), [texts[(i * B + b) % len(texts)] for b in range(B)])
            for i in range(n)]


def _raise(*a, **k):
    raise AssertionError("the host WER route was taken")


@pytest.mark.parametrize("opt,alpha", [("pgd", "0"), ("adam", "0"), ("pgd", "1e-6")])
def test_train_epoch_and_evaluate_equal_the_host_route(opt, alpha, monkeypatch):
    from paa_amd import arch as A, synth
    from paa_amd.core import loss_helpers as LH
    from paa_amd.model import PaaModel
    from paa_amd.training_utils import build, evaluation, train
    a = A.tiny()
    B, L = 3, 8000
    loader = _loader(4, B, L)
    res = {}
    for flag in (False, True):
        args = _args(["--optimizer_type", opt, "--norm_type", "linf", "--linf_size", "0.01", "--masking_loss_alpha", alpha]
                     + (["--device_wer"] if flag else []))
        m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
        p = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L)
        optimizer = None
        if opt == "adam":
            p = torch.nn.Parameter(p)
            optimizer, _ = build.create_optimizer(args, p)
        with monkeypatch.context() as mp_:
            if flag:
                mp_.setattr(LH, "wer_texts", _raise)               # the device route decodes nothing on the host
            out = []
            for epoch in range(2):
                r = train.train_epoch(args, loader, p, m, epoch, None, None, None, None, optimizer)
                p = r.p
                out.append((r.avg_ctc, r.avg_wer, r.avg_masking_loss))
            ev_c = evaluation.evaluate(args, loader, 0, m, None, None, perturbed=False)
            ev_p = evaluation.evaluate(args, loader, p, m, None, None, perturbed=True)
        torch.cuda.synchronize()
        res[flag] = (out, (ev_c.ctc, ev_c.wer), (ev_p.ctc, ev_p.wer), p.detach().clone())
    print(res[True][:3])
    assert res[True][:3] == res[False][:3]                           # exact: integers and the same float32 sums
    assert torch.equal(res[True][3], res[False][3])
    assert res[True][0][0][1] > 0 and (alpha == "0" or res[True][0][0][2] is not None)


def test_train_epoch_host_route_conditions(monkeypatch, caplog):
    """--device_wer with a wer_metric object, or with references over the row cap, keeps the host route and says so once."""
    from paa_amd import arch as A, synth
    from paa_amd.model import PaaModel
    from paa_amd.training_utils import train
    a = A.tiny()
    B, L = 2, 8000
    loader = _loader(2, B, L)
    metric = types.SimpleNamespace(compute=lambda predictions, references: 0.25)
    args = _args(["--norm_type", "linf", "--device_wer"])
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    p = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L)
    with caplog.at_level("WARNING"):
        r = train.train_epoch(args, loader, p.clone(), m, 0, None, None, metric, None, None)
    assert r.avg_wer == 0.25 and not m._stepper.device_wer
    assert "a wer_metric object is given" in caplog.text
    # references over the row cap: "hello there" needs 12 entries
    from paa_amd.core import loss_helpers as LH
    from paa_amd.training_utils import evaluation
    monkeypatch.setattr(LH, "R_CAP", 8)
    assert LH.encode_refs(["ab cd"]) is not None and LH.encode_refs(["hello there"]) is None
    plain = _args(["--norm_type", "linf"])
    m2 = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    want = train.train_epoch(plain, loader, p.clone(), m2, 0, None, None, None, None, None)
    m3 = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    with caplog.at_level("WARNING"):
        got = train.train_epoch(args, loader, p.clone(), m3, 0, None, None, None, None, None)
    assert m3._stepper.device_wer and m3._stepper.r_cap == 8 and "needs more than 8 entries" in caplog.text
    assert (got.avg_ctc, got.avg_wer) == (want.avg_ctc, want.avg_wer) and torch.equal(got.p, want.p)
    ev_want = evaluation.evaluate(plain, loader, want.p, m2, None, None, perturbed=True)
    ev_got = evaluation.evaluate(args, loader, got.p, m3, None, None, perturbed=True)
    assert (ev_got.ctc, ev_got.wer) == (ev_want.ctc, ev_want.wer)


def test_attack_clips_records_equal(monkeypatch):
    from paa_amd import arch as A, attack_clips, synth
    from paa_amd.core import loss_helpers as LH
    from paa_amd.model import PaaModel
    a = A.tiny()
    B, L = 3, 8000
    x = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    recs = {}
    for mode in ("untargeted", "targeted"):
        for flag in (False, True):
            ap = attack_clips.create_arg_parser()
            args = ap.parse_args(["--arch", "tiny", "--dtype", "fp32", "--silent", "--optimizer_type", "pgd", "--norm_type", "linf",
                                  "--linf_size", "0.01", "--lr", "1e-3", "--pgd_steps", "3", "--attack_mode", mode, "--target", "ab",
                                  "--target_reps", "2"] + (["--device_wer"] if flag else []))
            args.device = "cuda"
            m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
            with monkeypatch.context() as mp_:
                if flag:
                    mp_.setattr(LH, "wer_texts", _raise)
                recs[(mode, flag)] = attack_clips.attack_batch(m, None, args, x, TEXTS[:B], [0, 1, 2], None, None)[0]
        assert recs[(mode, True)] == recs[(mode, False)]
        assert ("target_wer" in recs[(mode, True)][0]) == (mode == "targeted")


if __name__ == "__main__":
    _rccl_child()
