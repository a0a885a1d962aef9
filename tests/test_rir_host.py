"""No-GPU checks of the room-response layer: the float64 references of tests/rir_ref.py against torch conv1d and
its autograd gradient, the pinned draw of the room index, the synthetic bank, banks from files, the parser's flags, the on / off
rule, every refusal that needs no GPU and the C-ABI entries."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import place_ref as PR
import rir_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_rir_draw", "paa_rir_apply")


@pytest.mark.parametrize("B,L,K", [(1, 1, 1), (2, 257, 5), (2, 300, 512)])
def test_references_vs_conv1d_and_autograd(B, L, K):
    rng = np.random.default_rng(B * 100000 + L * 1000 + K)
    N = 3
    bank, x, G = rng.standard_normal((N, K)), rng.standard_normal((B, L)), rng.standard_normal((B, L))
    index = [2, 0][:B]
    xt = torch.tensor(x, requires_grad=True)
    # conv1d correlates: flip the response and pad K - 1 zeros in front for the causal convolution with zero history
    w = torch.tensor(bank[index][:, ::-1].copy()).view(B, 1, K)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(xt.view(1, B, L), (K - 1, 0)), w, groups=B).view(B, L)
    (y * torch.tensor(G)).sum().backward()
    got = RR.apply64(bank, index, x)
    scale = np.abs(bank).sum() * np.abs(x).max()
    np.testing.assert_allclose(got, y.detach().numpy(), rtol=0, atol=1e-13 * scale)
    adj = RR.adjoint64(bank, index, G)
    np.testing.assert_allclose(adj, xt.grad.numpy(), rtol=0, atol=1e-13 * np.abs(bank).sum() * np.abs(G).max())
    # <apply(x), G> = <x, adjoint(G)>
    assert abs(float((got * G).sum()) - float((x * adj).sum())) <= 1e-12 * float(np.abs(got * G).sum() + 1e-300)
    # the definition, term by term, at a few outputs
    for b in range(B):
        h = bank[index[b]]
        for i in sorted({0, L // 2, L - 1}):
            assert got[b, i] == pytest.approx(sum(h[k] * x[b, i - k] for k in range(min(K - 1, i) + 1)), rel=1e-12, abs=1e-13)
            assert adj[b, i] == pytest.approx(sum(h[k] * G[b, i + k] for k in range(min(K - 1, L - 1 - i) + 1)), rel=1e-12, abs=1e-13)
    # indices outside [0, N) are reduced modulo N
    assert np.array_equal(RR.apply64(bank, [i + N for i in index], x), got) and np.array_equal(RR.apply64(bank, [i - N for i in index], x), got)


INDEX_TABLE = {1: [[0, 0, 0], [0, 0, 0], [0, 0, 0]],
               3: [[0, 0, 1], [2, 2, 2], [1, 2, 1]],
               64: [[17, 1, 40], [48, 58, 48], [24, 59, 38]]}


@pytest.mark.parametrize("N", [1, 3, 64])
def test_index_table(N):
    got = [[RR.draw_room(5, step, clip, 0, N) for clip in range(3)] for step in range(3)]
    assert got == INDEX_TABLE[N]
    assert RR.draw(5, 1, 1, 2, 0, N).tolist() == INDEX_TABLE[N][1][1:]
    # disjoint from placement's stream by construction: the counters differ in word 3
    assert PR.philox4x32_10((0, 0, 0, 1), (5, 0)) != PR.draw_raw(5, 0, 0, 0)
    if N == 64:
        assert [RR.draw_room(5, 0, c, 1, N) for c in range(3)] != INDEX_TABLE[N][0]          # the evaluation stream draws its own
        assert [RR.draw_room(6, 0, c, 0, N) for c in range(3)] != INDEX_TABLE[N][0]


def test_synthetic_bank():
    from paa_amd.training_utils import rir
    N, K, sr, lo, hi, D = 6, 3000, 16000, 0.2, 0.6, 6.0
    a = rir.synthetic_bank(N, K, sr, lo, hi, D, 5)
    b = rir.synthetic_bank(N, K, sr, lo, hi, D, 5)
    assert a.dtype == np.float32 and a.shape == (N, K) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.all(a[:, 0] == np.float32(1.0)) and np.isfinite(a).all()
    tail = (a[:, 1:].astype(np.float64) ** 2).sum(axis=1)
    np.testing.assert_allclose(tail, 10.0 ** (-D / 10.0), rtol=1e-6)
    rt = rir.synthetic_rt60(N, lo, hi, 5)
    assert rt.shape == (N,) and np.all(rt >= lo) and np.all(rt <= hi) and len(set(rt.tolist())) == N
    c = rir.synthetic_bank(N, K, sr, lo, hi, D, 6)
    assert not np.array_equal(a, c)                                               # another seed: another bank
    assert not np.array_equal(rir.synthetic_rt60(N, lo, hi, 5), rir.synthetic_rt60(N, lo, hi, 6))
    one = rir.synthetic_bank(2, 1, sr, lo, hi, D, 5)                              # K = 1: the direct path alone
    assert one.shape == (2, 1) and np.all(one == 1.0)
    # LO = HI: the envelope exp(-3 ln10 k / (rt60 sr)) is known; divided out, the tail is stationary (scaled normals)
    fixed = rir.synthetic_bank(2, 4000, sr, 0.25, 0.25, 0.0, 5).astype(np.float64)
    assert np.all(rir.synthetic_rt60(2, 0.25, 0.25, 5) == 0.25)
    k = np.arange(1, 4000)
    env = np.exp(-3.0 * np.log(10.0) * k / (0.25 * sr))
    flat = fixed[:, 1:] / env                                                     # the scaled normals
    assert abs(np.log((flat[:, 2000:] ** 2).mean() / (flat[:, :1999] ** 2).mean())) < 0.2


def test_bank_from_a_file(tmp_path):
    from paa_amd.training_utils import rir
    good = np.arange(12, dtype=np.float64).reshape(3, 4) / 7
    np.save(tmp_path / "good.npy", good)
    torch.save(torch.tensor(good, dtype=torch.float32), tmp_path / "good.pt")
    for name in ("good.npy", "good.pt"):
        b = rir.load_bank(str(tmp_path / name))
        assert b.dtype == np.float32 and np.array_equal(b, good.astype(np.float32))                # as it is
    a = _args(rir_bank=str(tmp_path / "good.npy"))
    assert rir.rir_on(a) and rir.suffix(a) == "_rir3x4"
    assert rir.results_extra(a) == {"rir_bank": str(tmp_path / "good.npy"), "rir_count": 3, "rir_taps": 4}
    bad = {"nan.npy": np.array([[1.0, np.nan]]), "inf.npy": np.array([[1.0, np.inf]]), "dim1.npy": np.ones(5), "dim3.npy": np.ones((2, 2, 2)),
           "long.npy": np.ones((1, 16385), dtype=np.float32), "int.npy": np.ones((2, 3), dtype=np.int32)}
    for name, arr in bad.items():
        np.save(tmp_path / name, arr)
        with pytest.raises(ValueError, match=re.escape(name)):
            rir.load_bank(str(tmp_path / name))
    np.save(tmp_path / "edge.npy", np.ones((1, 16384), dtype=np.float32))
    assert rir.load_bank(str(tmp_path / "edge.npy")).shape == (1, 16384)
    with pytest.raises(ValueError, match="missing.npy"):
        rir.load_bank(str(tmp_path / "missing.npy"))
    (tmp_path / "bank.txt").write_text("1 2 3")
    with pytest.raises(ValueError, match="bank.txt"):
        rir.load_bank(str(tmp_path / "bank.txt"))
    torch.save({"h": torch.ones(2, 2)}, tmp_path / "dict.pt")
    with pytest.raises(ValueError, match="dict.pt"):
        rir.load_bank(str(tmp_path / "dict.pt"))


def test_parser_defaults_and_flags():
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args([])
    assert a.rir_bank == "none" and a.rir_count == 64 and a.rir_taps == 4096 and list(a.rir_rt60) == [0.2, 0.6]
    assert a.rir_drr_db == 6.0 and a.rir_seed is None
    a = parser.create_arg_parser().parse_args(["--rir_bank", "synthetic", "--rir_count", "8", "--rir_taps", "1024", "--rir_rt60", "0.3",
                                               "0.5", "--rir_drr_db", "3", "--rir_seed", "9"])
    assert (a.rir_bank, a.rir_count, a.rir_taps, list(a.rir_rt60), a.rir_drr_db, a.rir_seed) == ("synthetic", 8, 1024, [0.3, 0.5], 3.0, 9)
    for bad in (["--rir_count", "0"], ["--rir_taps", "0"], ["--rir_taps", "16385"], ["--rir_rt60", "0.2"], ["--rir_rt60", "0", "0.5"],
                ["--rir_drr_db", "100"]):
        with pytest.raises(SystemExit):
            parser.create_arg_parser().parse_args(bad)


def _args(**kw):
    from paa_amd.training_utils import parser
    a = parser.create_arg_parser().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_on_off_rule():
    from paa_amd.training_utils import place, rir
    assert not rir.rir_on(types.SimpleNamespace())                             # callers that never heard of the flags
    assert not rir.rir_on(_args())
    assert not rir.rir_on(_args(rir_count=8, rir_taps=100))                    # the bank flag alone switches the mode on
    on = _args(rir_bank="synthetic", rir_count=4, rir_taps=100)
    assert rir.rir_on(on) and not place.placement_on(on)                       # placement keeps its own meaning
    assert rir.suffix(_args()) == "" and rir.results_extra(_args()) == {}
    assert rir.suffix(on) == "_rir4x100" and place.suffix(on) == "" and place.results_extra(on, 16000) == {}
    assert rir.results_extra(on) == {"rir_bank": "synthetic", "rir_count": 4, "rir_taps": 100}
    bank = rir.bank_of(on)
    assert bank.shape == (4, 100) and np.array_equal(bank, rir.synthetic_bank(4, 100, 16000, 0.2, 0.6, 6.0, 5))   # rir_seed: --seed
    assert not np.array_equal(rir.bank_of(_args(rir_bank="synthetic", rir_count=4, rir_taps=100, rir_seed=6)), bank)
    assert rir.draw_seed(_args(seed=11)) == 11


def test_refusals_without_gpu():
    from paa_amd import attack_clips
    from paa_amd.training_utils import rir
    from paa_amd.training_utils.pgd import PgdStepper
    model = types.SimpleNamespace(device=torch.device("cpu"), max_batch=2, length=16000)
    small = dict(rir_bank="synthetic", rir_count=2, rir_taps=16)
    # the masking norm / loss pair delta's frames with the clean clip's
    for a in (_args(norm_type="masking", **small), _args(norm_type="linf+masking", **small),
              _args(norm_type="linf", masking_loss_alpha=0.5, **small)):
        with pytest.raises(NotImplementedError, match="masking"):
            rir.check(a)
        with pytest.raises(NotImplementedError, match="masking"):
            rir.check_flags(a)                                                # the runner's check before any collective
        with pytest.raises(NotImplementedError, match="masking"):
            PgdStepper(model, a, 16000)                                       # raised before anything touches a device
    rir.check(_args(norm_type="masking"))                                     # the mode off: nothing to refuse
    rir.check(_args(norm_type="masking"), eager_adam=True)
    for n in ("snr", "tv", "linf+tv"):                                        # Lp = L: fine
        rir.check(_args(norm_type=n, **small))
    # the eager-Adam route
    with pytest.raises(NotImplementedError, match="device step"):
        rir.check(_args(norm_type="linf", **small), eager_adam=True)
    # values outside the flags' ranges reaching the stepper through a hand-built namespace
    for kw, name in ((dict(rir_count=0), "rir_count"), (dict(rir_taps=0), "rir_taps"), (dict(rir_taps=16385), "rir_taps"),
                     (dict(rir_rt60=[0.5, 0.2]), "rir_rt60"), (dict(rir_rt60=[0.0, 0.2]), "rir_rt60"), (dict(rir_rt60=[0.2]), "rir_rt60"),
                     (dict(rir_drr_db=100.0), "rir_drr_db")):
        a = _args(norm_type="linf", **{**small, **kw})
        with pytest.raises(ValueError, match=name):
            rir.check(a)
        with pytest.raises(ValueError, match=name):
            PgdStepper(model, a, 16000)
    with pytest.raises(ValueError, match="no_such_bank.npy"):
        PgdStepper(model, _args(norm_type="linf", rir_bank="/no_such_bank.npy"), 16000)
    # a p_length of its own still needs placement on
    with pytest.raises(ValueError, match="p_length"):
        PgdStepper(model, _args(norm_type="linf", **small), 16000, p_length=4096)
    # per-clip perturbations have no room responses
    with pytest.raises(NotImplementedError, match="per-clip"):
        attack_clips.main(attack_clips.create_arg_parser().parse_args(["--rir_bank", "synthetic"]))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from paa_amd import _lib
    return _lib


def test_new_entries_declared_exported_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "paa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(paa_[a-z0-9_]+)\s*\(", hdr))
    L = lib.lib()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in lib.exported_symbols(), name
        assert hasattr(L, name), name
    assert re.search(r"#define\s+PAA_RIR_MAX_TAPS\s+16384\b", hdr)
    from paa_amd.training_utils import rir
    assert rir.MAX_TAPS == 16384


def test_new_entries_refuse_before_any_launch(lib):
    L = lib.lib()
    d, e = C.c_void_p(1 << 20), C.c_void_p(1 << 24)        # never dereferenced: the arguments are refused first
    ARG = lib.PAA_ERR_ARG
    assert L.paa_rir_draw(5, None, 0, 0, 2, 4, d, None) == ARG
    assert L.paa_rir_draw(5, d, 0, 0, 2, 4, None, None) == ARG
    assert L.paa_rir_draw(5, d, 0, 0, 0, 4, d, None) == ARG
    assert L.paa_rir_draw(5, d, 0, 0, 2, 0, d, None) == ARG
    assert b"paa_rir_draw" in L.paa_last_error()
    for k in range(4):
        a = [d, d, d, e]
        a[k] = None
        assert L.paa_rir_apply(a[0], 4, 8, a[1], a[2], a[3], 2, 100, 0, None) == ARG
    for N_, K_, B_, L_ in ((0, 8, 2, 100), (4, 0, 2, 100), (4, -1, 2, 100), (4, 16385, 2, 100), (4, 8, 0, 100), (4, 8, 2, 0)):
        for adj in (0, 1):
            assert L.paa_rir_apply(d, N_, K_, d, d, e, B_, L_, adj, None) == ARG
    assert L.paa_rir_apply(d, 4, 16385, d, d, e, 2, 100, 0, None) == ARG and b"16384" in L.paa_last_error()
    # overlapping in / out: identical, and shifted by less than B * L floats either way
    for off in (0, 4, 2 * 100 * 4 - 4, -(2 * 100 * 4 - 4)):
        assert L.paa_rir_apply(d, 4, 8, d, e, C.c_void_p((1 << 24) + off), 2, 100, 0, None) == ARG
        assert b"overlap" in L.paa_last_error()
