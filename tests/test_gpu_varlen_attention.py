"""-m gpu: the fused attention kernels with a per-clip key count (paa_attn_*_len, csrc/attention.hip).

Nothing here has a tolerance: clip b at key count klen_b does, per (clip, head, 128-position block), the arithmetic the
mask-free entries do for that clip alone at T = klen_b, so the bits must agree; rows [klen_b, T) of ctx and dqkv are zero
bits; rows [T, P) keep the sentinel; klen = NULL is the existing entry."""
import numpy as np
import pytest
import torch

import attn_ref as R
from paa_amd import _lib
from test_gpu_attention import _dev16, _same, _sentinel16, _sentinel32, run_attention

pytestmark = pytest.mark.gpu

# two 128-position blocks, three 64-key tiles; klen on, just past and far below the block / tile edges
B, NH, T = 3, 2, 160
P, TP = T + 5, 160
KLENS = ([160, 65, 1], [128, 64, 33])
H = NH * R.HD
_cache = {}


def _inputs(mode):
    if mode not in _cache:
        _cache[mode] = R.build_inputs(B, NH, T, P, TP, mode == "split", seed=4242)
    return _cache[mode]


def run_len(inp, klen):
    """Forward then backward through the _len entries (klen: list or None = NULL pointer); outputs start as the sentinel."""
    split = inp["qkv_lo"] is not None
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    kl = None if klen is None else torch.tensor(klen, dtype=torch.int32, device="cuda")
    qh, dh = _dev16(inp["qkv_hi"]), _dev16(inp["do_hi"])
    ch, gh = _sentinel16(B * P, H), _sentinel16(B * P, 3 * H)
    lse, delta = _sentinel32(B * NH, TP), _sentinel32(B * NH, TP)
    if split:
        ql, dl = _dev16(inp["qkv_lo"]), _dev16(inp["do_lo"])
        cl, gl = _sentinel16(B * P, H), _sentinel16(B * P, 3 * H)
        _lib.check(L.paa_attn_fwd_split_len(p(qh), p(ql), p(ch), p(cl), p(lse), p(kl), B, T, P, TP, H, NH, st))
        _lib.check(L.paa_attn_bwd_split_len(p(qh), p(ql), p(ch), p(cl), p(lse), p(dh), p(dl), p(delta), p(gh), p(gl), p(kl),
                                            B, T, P, TP, H, NH, st))
    else:
        cl = gl = None
        _lib.check(L.paa_attn_fwd_len(p(qh), p(ch), p(lse), p(kl), B, T, P, TP, H, NH, st))
        _lib.check(L.paa_attn_bwd_len(p(qh), p(ch), p(lse), p(dh), p(delta), p(gh), p(kl), B, T, P, TP, H, NH, st))
    torch.cuda.synchronize()
    host16 = lambda t: None if t is None else t.cpu().numpy().view(np.uint16)
    return {"ctx_hi": host16(ch), "ctx_lo": host16(cl), "dqkv_hi": host16(gh), "dqkv_lo": host16(gl),
            "lse": lse.cpu().numpy(), "delta": delta.cpu().numpy()}


PLANES = ("ctx_hi", "ctx_lo", "dqkv_hi", "dqkv_lo")


@pytest.mark.parametrize("mode", ["bf16", "split"])
@pytest.mark.parametrize("klen", KLENS, ids=lambda k: "-".join(map(str, k)))
def test_rows_below_klen_equal_the_clip_alone(mode, klen):
    inp = _inputs(mode)
    out = run_len(inp, klen)
    for b, kb in enumerate(klen):
        sub = {k: (None if v is None else v.reshape(B, P, -1)[b]) for k, v in inp.items() if k.endswith(("_hi", "_lo"))}
        one = run_attention(sub, 1, NH, kb, P, TP)          # the existing entries, this clip alone, scalar T = klen_b
        for name in PLANES:
            if out[name] is None:
                continue
            got = out[name].reshape(B, P, -1)[b]
            assert np.array_equal(got[:kb], one[name][:kb]), (b, name, "rows < klen")
            if name.startswith(("ctx", "dqkv")):
                assert (got[kb:T] == 0).all(), (b, name, "rows [klen, T) must be zero bits")
            assert (got[T:] == R.NAN16).all(), (b, name, "rows [T, P) must keep the sentinel")
        for name in ("lse", "delta"):
            got = out[name].reshape(B, NH, TP)[b]
            assert _same(np.ascontiguousarray(got[:, :kb]), np.ascontiguousarray(one[name][:, :kb])), (b, name)


@pytest.mark.parametrize("mode", ["bf16", "split"])
def test_null_klen_is_the_existing_entry(mode):
    inp = _inputs(mode)
    ref = run_attention(inp, B, NH, T, P, TP)
    out = run_len(inp, None)
    for name, a in ref.items():
        assert _same(a, out[name]), name
    full = run_len(inp, [T] * B)                             # klen = T for every clip: the same bits again
    for name, a in ref.items():
        assert _same(a, full[name]), name


@pytest.mark.parametrize("mode", ["bf16", "split"])
def test_two_calls_give_the_same_bits(mode):
    inp = _inputs(mode)
    a, b = run_len(inp, KLENS[0]), run_len(inp, KLENS[0])
    for name in a:
        assert _same(a[name], b[name]), name


def test_out_of_range_klen_is_clamped():
    """The device clamps klen to [1, T]: 0 and a negative count act as 1, a count past T as T (never an out-of-bounds index)."""
    inp = _inputs("bf16")
    got, ref = run_len(inp, [T + 1000, 0, -7]), run_len(inp, [T, 1, 1])
    for name in got:
        assert _same(got[name], ref[name]), name
