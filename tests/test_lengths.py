"""Clip lengths off the 8000-sample grid (oracle.gen_cases.ODD_LENGTHS), no GPU: the list covers every tail class of the conv stack
and attention, and at each of its lengths the oracle equals HF's Wav2Vec2ForCTC in float64 (logits, CTC loss, d loss / d waveform),
so the GPU tests that compare the HIP path with the oracle there rest on a pinned reference."""
import numpy as np
import pytest
import torch

from gemm_ref import padded_rows
from oracle import pgd as opgd, wav2vec2 as OW
from oracle.gen_cases import ODD_LENGTHS, PGD_TEXTS, cli_to_args
from paa_amd import arch as A, synth

LENGTHS = [L for L, _ in ODD_LENGTHS]
DG_T, C0_TCH, C0_GCH = 32, 128, 2048          # conv0_dgrad.hip / model_kernels.hip tile sizes


def length_classes(a, L):
    """The tail of every hand-written loop the clip length reaches (see the table above ODD_LENGTHS)."""
    T, P = padded_rows(a, L)
    return dict(t0_dgrad=T[0] % DG_T, t0_walk=(T[0] % C0_TCH) % 4, gram_tail=(T[0] - 1) % C0_GCH + 1, pad0=P[0] - T[0],
                uncovered=L - ((T[0] - 1) * a.conv_stride[0] + a.conv_kernel[0]), te_mod=T[-1] % 32, te=T[-1], l_mod4=L % 4)


def test_padded_layout_restated():
    """padded_rows restates csrc/model.hip's layout search: P_last = T_last + extra with the smallest extra >= 1 for which
    P_{i-1} = stride_i * P_i >= T_{i-1} holds at every layer."""
    for a in (A.BASE, A.tiny()):
        for L in LENGTHS:
            T, P = padded_rows(a, L)
            assert T == a.feat_lengths(L)
            assert all(p >= t for p, t in zip(P, T)), L
            assert all(P[i - 1] == a.conv_stride[i] * P[i] for i in range(1, len(P))), L
            extra = P[-1] - T[-1]
            for e in range(1, extra):           # no smaller extra gives a valid layout
                p, ok = T[-1] + e, True
                for i in range(len(T) - 1, -1, -1):
                    ok &= p >= T[i]
                    p *= a.conv_stride[i]
                assert not ok, (L, e)


def test_odd_lengths_cover_every_tail_class():
    """A later edit of ODD_LENGTHS must not drop a class: every residue of the conv0 / attention tails is present."""
    assert len(set(LENGTHS)) == len(LENGTHS) and min(LENGTHS) >= 400 and 8000 in LENGTHS
    assert all(why for _, why in ODD_LENGTHS)
    cls = [length_classes(A.BASE, L) for L in LENGTHS]
    got = {k: {c[k] for c in cls} for k in cls[0]}
    assert {0, 1, 18, 31} <= got["t0_dgrad"], got["t0_dgrad"]            # no tail, 31 zeroed rows, a middle, one zeroed row
    assert {0, 1, 2, 3} <= got["t0_walk"], got["t0_walk"]
    assert {1, C0_GCH} <= got["gram_tail"], got["gram_tail"]              # one-frame gram chunk, full last chunk
    assert 0 in got["pad0"] and max(got["pad0"]) >= 63, got["pad0"]       # P0 == T0, and up to 63 padded conv0 rows
    assert {0, 1, 2, 3, 4} <= got["uncovered"], got["uncovered"]          # every count of samples no conv0 window covers
    assert {0, 1} <= got["te_mod"] and 1 in got["te"], got["te_mod"]     # Tp == T_e, one row past a block, a one-frame clip
    assert {0, 1, 2, 3} <= got["l_mod4"], got["l_mod4"]
    # the 8000-multiples the rest of the suite runs at sit in one class of each tail
    for L in (8000, 16000, 32000, 160000, 480000):
        c = length_classes(A.BASE, L)
        assert (c["t0_dgrad"], c["t0_walk"], c["uncovered"], c["l_mod4"]) == (31, 3, 0, 0), (L, c)


def texts_for(a, L, B):
    """PGD_TEXTS, or a one-token label where the clip has a single frame (T_e = 1: a longer label has no CTC alignment)."""
    return ["a"] * B if a.feat_lengths(L)[-1] < 8 else PGD_TEXTS[:B]


def _hf_vs_oracle(a, L, B):
    pytest.importorskip("transformers")
    from hf_util import hf_model
    sdn = A.rule_weights(a)
    hf = hf_model(a, sdn).double()
    sd = {k: v.double() for k, v in OW.to_torch(sdn).items()}
    args = cli_to_args("snr", [])
    labels = opgd.make_labels(texts_for(a, L, B), args, B)
    clean = torch.from_numpy(synth.clean_audio(B, L)).double()
    p0 = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).double()
    out = []
    for run in ("oracle", "hf"):
        p = p0.clone().requires_grad_(True)
        x = (clean + p).clamp(-1, 1)
        if run == "oracle":
            loss, logits = OW.forward(sd, a, x, labels)
        else:
            o = hf(input_values=x, labels=labels)
            loss, logits = o.loss, o.logits
        loss.backward()
        out.append((float(loss.detach()), logits.detach().numpy(), p.grad.numpy().copy()))
    (l_o, lg_o, g_o), (l_h, lg_h, g_h) = out
    T = a.feat_lengths(L)
    assert lg_o.shape == lg_h.shape == (B, T[-1], a.vocab_size)
    assert np.isfinite(l_o) and np.isfinite(l_h)
    e_lg = np.abs(lg_o - lg_h).max() / np.abs(lg_h).max()
    e_g = np.abs(g_o - g_h).max() / np.abs(g_h).max()
    # log_softmax runs in float32 in both (modeling_wav2vec2.py's CTC branch): loss and gradient carry its rounding
    assert e_lg < 1e-12, (L, e_lg)
    assert abs(l_o - l_h) <= 1e-6 * abs(l_h), (L, l_o, l_h)
    assert e_g < 1e-5, (L, e_g)
    tail = (T[0] - 1) * a.conv_stride[0] + a.conv_kernel[0]
    assert np.all(g_o[:, tail:] == 0) and np.all(g_h[:, tail:] == 0)    # no conv0 window covers these samples
    assert np.array_equal(g_o == 0, g_h == 0)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("variant", ["group", "layer_stable"])
def test_oracle_vs_hf_at_length(variant, L):
    a = A.tiny("group", False) if variant == "group" else A.tiny("layer", True)
    _hf_vs_oracle(a, L, 2)


def test_oracle_vs_hf_base_odd_length():
    _hf_vs_oracle(A.BASE, 10563, 2)
