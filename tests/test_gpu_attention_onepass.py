"""-m gpu: the one-pass attention backward (k_attn_bwd_one + k_attn_dq_finish, csrc/attention.hip) against float64, against
the dQ / dK/dV kernel pair, in length mode, for reproducibility and for its dispatch rule.

Inputs, the float64 reference and every bound come from tests/test_gpu_attention.py and tests/attn_ref.py: the one-pass path
is held to what the kernel pair is held to.  The backward entries own no workspace; whenever they take the one-pass path they
allocate one filled with NaN bits, so every call here also checks that no partial is read that was never written."""
import numpy as np
import pytest
import torch

import attn_ref as R
from paa_amd import _lib
from test_gpu_attention import (KAPPA_SAT, SAT, T1_BOUND, TIGHT, _dev16, _err, _head_outputs, _sentinel16, _sentinel32)

pytestmark = pytest.mark.gpu

B, NH = 2, 2
H = NH * R.HD
# 1: one key, one query; 31 / 32 / 33: a ragged, a full and a second query tile; 255 / 256 / 257: the key-block edge (257: a
# second block holding one key); 499: the model's 10 s clips; 512: the last two-block size; 513: a third block
EDGES = [1, 31, 32, 33, 255, 256, 257, 499, 512, 513]
TWO_KERNELS, ONE_PASS = 1, 2
PLANES = ("dqkv_hi", "dqkv_lo", "delta")
# A clip of ONE key (T = 1, or klen = 1 inside a longer call): the exact dQ and dK are 0 and a kernel's are dP - delta, two
# roundings of one 64-term sum, normalised as in test_gpu_attention.py and held to its T1_BOUND.  In length mode the one-pass
# result is held to that bound against what the kernel pair gives on the same inputs (the two differ only in the order delta is
# summed in), as the varlen tests hold a clip to the kernels' own result for the clip alone; both figures are printed.


def _dims(T):
    return T, T + 3, -(-T // 32) * 32


@pytest.fixture(autouse=True)
def _automatic_mode_afterwards():
    yield
    _lib.lib().paa_attn_bwd_config(0)


_inputs, _runs, _refs = {}, {}, {}


def inputs(mode, T):
    if (mode, T) not in _inputs:
        _, P, Tp = _dims(T)
        _inputs[mode, T] = R.build_inputs(B, NH, T, P, Tp, mode == "split", seed=9000 + T)
    return _inputs[mode, T]


def reference(mode, T, b, h, n):
    """float64 reference of head (b, h) over the clip's first n positions; computed once per case and shared."""
    if (mode, T, b, h, n) not in _refs:
        inp = inputs(mode, T)
        q, k, v = (x[:n] for x in R.head_slices(inp["qkv"][b], NH, h))
        _refs[mode, T, b, h, n] = (q, k, v, inp["do"][b][:n, h * R.HD:(h + 1) * R.HD], R.attn_ref(q, k, v, inp["do"][b][:n, h * R.HD:(h + 1) * R.HD]))
    return _refs[mode, T, b, h, n]


def run(mode, T, bwd_mode, klen=None):
    """Forward, then the backward in path `bwd_mode`, through the _len entries (klen None = the null pointer).  Returns the
    device tensors (every output starts as the NaN sentinel) and the number of one-pass dispatches the backward made."""
    inp = inputs(mode, T)
    _, P, Tp = _dims(T)
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    kl = None if klen is None else torch.tensor(klen, dtype=torch.int32, device="cuda")
    qh, dh = _dev16(inp["qkv_hi"]), _dev16(inp["do_hi"])
    ch, gh = _sentinel16(B * P, H), _sentinel16(B * P, 3 * H)
    lse, delta = _sentinel32(B * NH, Tp), _sentinel32(B * NH, Tp)
    cl = gl = None
    L.paa_attn_bwd_config(bwd_mode)
    if mode == "split":
        ql, dl = _dev16(inp["qkv_lo"]), _dev16(inp["do_lo"])
        cl, gl = _sentinel16(B * P, H), _sentinel16(B * P, 3 * H)
        _lib.check(L.paa_attn_fwd_split_len(p(qh), p(ql), p(ch), p(cl), p(lse), p(kl), B, T, P, Tp, H, NH, st))
        _lib.check(L.paa_attn_bwd_split_len(p(qh), p(ql), p(ch), p(cl), p(lse), p(dh), p(dl), p(delta), p(gh), p(gl), p(kl),
                                            B, T, P, Tp, H, NH, st))
    else:
        _lib.check(L.paa_attn_fwd_len(p(qh), p(ch), p(lse), p(kl), B, T, P, Tp, H, NH, st))
        _lib.check(L.paa_attn_bwd_len(p(qh), p(ch), p(lse), p(dh), p(delta), p(gh), p(kl), B, T, P, Tp, H, NH, st))
    torch.cuda.synchronize()
    n = L.paa_attn_bwd_config(0)
    return {"ctx_hi": ch, "ctx_lo": cl, "dqkv_hi": gh, "dqkv_lo": gl, "lse": lse, "delta": delta.view(torch.int32)}, n


def cached(mode, T, bwd_mode):
    """One run per (precision, T, path), shared by the tests below and never modified."""
    if (mode, T, bwd_mode) not in _runs:
        _runs[mode, T, bwd_mode] = run(mode, T, bwd_mode)
    return _runs[mode, T, bwd_mode]


def host(out):
    h = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    for k in ("ctx_hi", "ctx_lo", "dqkv_hi", "dqkv_lo"):
        h[k] = None if h[k] is None else h[k].view(np.uint16)
    h["delta"] = h["delta"].view(np.float32)
    return h


def check_against_float64(mode, T, out, klen=None, pair=None):
    """dQ, dK, dV and delta of every (clip, head) against float64 over the clip's first klen positions, with the bounds of
    test_attention_parity_sweep; rows [klen, T) of dqkv are zero bits, rows [T, P) and delta past klen keep the sentinel.
    pair: the kernel pair's outputs for the same call (length mode), the yardstick of a one-key clip."""
    inp = inputs(mode, T)
    _, P, Tp = _dims(T)
    klen = [T] * B if klen is None else klen
    bad, worst = [], {}

    def record(key, e, bound, what):
        worst[key] = max(worst.get(key, 0.0), e)
        if not e <= bound:
            bad.append(f"{what} {e:.2e} > {bound:.0e}")

    for name in ("dqkv_hi", "dqkv_lo"):
        if out[name] is None:
            continue
        g = out[name].reshape(B, P, 3 * H)
        assert (g[:, T:] == R.NAN16).all(), f"{name}: write into a pad row"
        for b in range(B):
            assert (g[b, klen[b]:T] == 0).all(), f"{name}: rows [klen, T) of clip {b} must be zero bits"
    delta = out["delta"].reshape(B, NH, Tp)
    for b in range(B):
        n = klen[b]
        assert (delta[b, :, n:].view(np.uint32) == R.NAN32).all(), "delta: write past klen"
        assert np.isfinite(delta[b, :, :n]).all(), "delta: NaN / Inf (or an unwritten entry) below klen"
        for h in range(NH):
            pat = inp["patterns"][b * NH + h]
            tag = f"({b},{h}) {pat}"
            q, k, v, do, ref = reference(mode, T, b, h, n)
            got = {t: x[:n] for t, x in _head_outputs(out, b, h, B, NH, T, P).items()}
            for t in ("dq", "dk", "dv"):
                assert np.isfinite(got[t]).all(), f"{tag} {t}: NaN / Inf (or an unwritten position) in rows < klen"
            prod = do * got["o"]
            record((pat, "delta"), float((np.abs(delta[b, h, :n] - prod.sum(1)) / np.abs(prod).sum(1)).max()), 1e-5, f"{tag} delta")
            for t in ("dq", "dk", "dv"):
                if n == 1 and t in ("dq", "dk"):
                    nat = R.SCALE * np.abs(do * v).sum() * np.abs(k if t == "dq" else q).max()
                    if pair is None:
                        record((pat, t), float(np.abs(got[t]).max() / nat), T1_BOUND[mode], f"{tag} {t} (one key)")
                    else:
                        two = _head_outputs(pair, b, h, B, NH, T, P)[t][:n]
                        print(f"ONEPASS {mode} T={T} {tag} {t} one key: one pass {np.abs(got[t]).max() / nat:.2e}, pair {np.abs(two).max() / nat:.2e}")
                        record((pat, t), float(np.abs(got[t] - two).max() / nat), T1_BOUND[mode], f"{tag} {t} (one key, against the pair)")
                elif t in ref["kappa"] and ref["kappa"][t] > KAPPA_SAT:
                    record((pat, t + "/sat"), float(_err(got[t], ref[t])), SAT[mode][t], f"{tag} {t} (saturated)")
                    record((pat, t + "/nat"), float(np.abs(got[t] - ref[t]).max() / ref["nat"][t].max()), TIGHT[mode][t],
                           f"{tag} {t} (saturated) against its natural scale")
                else:
                    record((pat, t), float(_err(got[t], ref[t])), TIGHT[mode][t], f"{tag} {t}")
            if pat == "flat" and not (got["dk"] == 0).all():
                bad.append(f"{tag}: dK not exactly 0")
    for (pat, t), e in sorted(worst.items()):
        print(f"ONEPASS {mode} T={T} klen={klen} {pat:13s} {t:10s} {e:.2e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("mode", ["bf16", "split"])
@pytest.mark.parametrize("T", EDGES)
def test_onepass_ragged_edges_against_float64(mode, T):
    out, n = cached(mode, T, ONE_PASS)
    assert n == 1, "the forced mode did not take the one-pass path"
    check_against_float64(mode, T, host(out))


@pytest.mark.parametrize("mode", ["bf16", "split"])
@pytest.mark.parametrize("T", [257, 499, 513])
def test_onepass_agrees_with_the_two_kernels(mode, T):
    """Same inputs through both paths: their difference stays within the bound each path is held to against float64 (for a
    saturated dQ / dK block that is SAT relative to the block and TIGHT relative to its natural scale, as in the parity sweep)."""
    _, P, Tp = _dims(T)
    (one, n1), (two, n2) = cached(mode, T, ONE_PASS), cached(mode, T, TWO_KERNELS)
    assert (n1, n2) == (1, 0)
    one, two = host(one), host(two)
    for b in range(B):
        for h in range(NH):
            a, r = _head_outputs(one, b, h, B, NH, T, P), _head_outputs(two, b, h, B, NH, T, P)
            ref = reference(mode, T, b, h, T)[4]
            for t in ("dq", "dk", "dv"):
                e = float(_err(a[t], r[t]))
                if t in ref["kappa"] and ref["kappa"][t] > KAPPA_SAT:
                    assert e <= SAT[mode][t], (b, h, t, "saturated", e)
                    e = float(np.abs(a[t] - r[t]).max() / ref["nat"][t].max())
                assert e <= TIGHT[mode][t], (b, h, t, e)
            prod = np.abs(inputs(mode, T)["do"][b][:, h * R.HD:(h + 1) * R.HD] * r["o"]).sum(1)
            d1, d2 = (x["delta"].reshape(B, NH, Tp)[b, h, :T] for x in (one, two))
            assert (np.abs(d1 - d2) / prod).max() <= 1e-5, (b, h, "delta")
    cols = lambda x, i: np.ascontiguousarray(x.reshape(B, P, 3 * H)[:, :T, i * H:(i + 1) * H])
    for i, t in ((1, "dK"), (2, "dV")):
        same = all(one[pl] is None or np.array_equal(cols(one[pl], i), cols(two[pl], i)) for pl in ("dqkv_hi", "dqkv_lo"))
        print(f"ONEPASS {mode} T={T}: {t} bit-equal to the two-kernel path: {same}")


# klen on the key-block edge, one key into the second block, and clips whose second block lies wholly beyond klen (1, 200, 256)
@pytest.mark.parametrize("mode", ["bf16", "split"])
@pytest.mark.parametrize("klen", [[1, None], [256, 257], [200, 256]], ids=["1-T", "256-257", "200-256"])
@pytest.mark.parametrize("T", [257, 499])
def test_onepass_length_mode(mode, T, klen):
    klen = [T if k is None else k for k in klen]
    out, n = run(mode, T, ONE_PASS, klen)
    assert n == 1
    pair = host(run(mode, T, TWO_KERNELS, klen)[0]) if 1 in klen else None
    check_against_float64(mode, T, host(out), klen, pair)


@pytest.mark.parametrize("mode", ["bf16", "split"])
@pytest.mark.parametrize("T", [499, 513])
def test_onepass_gives_the_same_bits_on_every_run(mode, T):
    """Two calls (each with a fresh NaN-filled workspace) agree bit for bit in dQ, dK, dV and delta."""
    a, _ = cached(mode, T, ONE_PASS)
    b, n = run(mode, T, ONE_PASS)
    assert n == 1
    for name in PLANES:
        assert a[name] is None and b[name] is None or torch.equal(a[name], b[name]), name


def test_dispatch_rule():
    """Automatic: one pass in split mode up to two key blocks (T <= 512), the kernel pair beyond and in bf16 mode (where one
    pass measured slower, profiles/attn_onepass_ab.txt); mode 1: always the kernel pair; mode 2: one pass everywhere."""
    assert run("split", 499, 0)[1] == 1
    assert run("split", 513, 0)[1] == 0
    assert run("bf16", 499, 0)[1] == 0
    assert run("split", 499, TWO_KERNELS)[1] == 0
    assert run("bf16", 513, ONE_PASS)[1] == 1
