"""-m gpu: each HIP kernel against a float64 / torch-fp32 statement of the same op, through the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gemm_ref import emulate
from gpu_util import dev, rel_err, run_gemm
from paa_amd import _lib

pytestmark = pytest.mark.gpu
TOL = {0: 1.5e-2, 1: 6e-5}      # bf16 operands | split-bf16 (fp32-parity) — relative to max|ref|


def _case(name, d, shapes, prec, seed=0, offs=None, zero_c=False):
    """shapes: operand name -> flat length.  Runs HIP and the numpy emulator on identical buffers."""
    rng = np.random.default_rng(seed)
    host = {k: rng.normal(size=n).astype(np.float32) for k, n in shapes.items()}
    if zero_c:
        host["C"][:] = 0
    bufs = {k: dev(v) for k, v in host.items()}
    dd = dict(d)
    dd["precision"] = prec
    names = {k: k for k in shapes}
    run_gemm({**dd, **names}, bufs, offs)
    ref = {k: v.astype(np.float64) for k, v in host.items()}
    o = offs or {}
    emulate(dd, ref["A"], ref["B"], ref["C"], a_off=o.get("A", 0), b_off=o.get("B", 0), c_off=o.get("C", 0),
            bias=ref.get("bias"), aux=ref.get("aux"), aux_off=o.get("aux", 0), residual=ref.get("residual"),
            res_off=o.get("residual", 0), C_pre=ref.get("C_pre"))
    e = rel_err(bufs["C"].cpu().numpy(), ref["C"])
    print(f"gemm[{name}] prec={prec} rel_err={e:.3e}")
    assert e < TOL[prec], name
    if "C_pre" in shapes:
        e2 = rel_err(bufs["C_pre"].cpu().numpy(), ref["C_pre"])
        print(f"gemm[{name}] C_pre rel_err={e2:.3e}")
        assert e2 < TOL[prec], name + ".C_pre"


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_plain_edges_bias_gelu(prec):
    M, N, K = 300, 200, 96
    _case("plain", dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, alpha=0.5, act=1), dict(A=M * K, B=N * K, C=M * N, bias=N, C_pre=M * N), prec)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_big_k(prec):
    M, N, K = 257, 384, 1536
    _case("bigk", dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N), dict(A=M * K, B=N * K, C=M * N), prec)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_conv_view_rowmask(prec):
    Cc, k, s, M = 32, 3, 2, 250
    rows = s * M + 8
    _case("convview", dict(M=M, N=Cc, K=k * Cc, lda=s * Cc, ldb=k * Cc, ldc=Cc, row_period=50, row_valid=49, act=1),
          dict(A=rows * Cc, B=Cc * k * Cc, C=M * Cc, C_pre=M * Cc), prec)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_k_tail_and_narrow(prec):
    M, N, K = 130, 48, 499
    _case("ktail", dict(M=M, N=N, K=K, lda=512, ldb=512, ldc=N), dict(A=M * 512, B=N * 512, C=M * N), prec)
    _case("n32", dict(M=200, N=32, K=64, lda=64, ldb=64, ldc=32), dict(A=200 * 64, B=32 * 64, C=200 * 32, bias=32), prec)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_transposed_operands(prec):
    T, hd, ld = 499, 64, 512
    # P V : A (T x T, ld 512) k-contig, B [K][N] with ldb 192
    _case("pv", dict(M=T, N=hd, K=T, lda=ld, ldb=192, b_kcontig=0, ldc=hd), dict(A=T * ld, B=T * 192, C=T * hd), prec)
    # P^T dO : A stored [K][M], B [K][N]
    _case("ptdo", dict(M=T, N=hd, K=T, lda=ld, a_kcontig=0, ldb=64, b_kcontig=0, ldc=192),
          dict(A=T * ld, B=T * 64, C=T * 192), prec, zero_c=True)
    # A^T with B k-contig
    _case("at_b", dict(M=100, N=130, K=72, lda=104, a_kcontig=0, ldb=72, ldc=130), dict(A=72 * 104, B=130 * 72, C=100 * 130), prec)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_batched_heads(prec):
    B, nh, T, hd, P = 2, 3, 70, 16, 71
    H3 = 3 * nh * hd
    Tp = 96
    d = dict(M=T, N=T, K=hd, lda=H3, ldb=H3, ldc=Tp, batch=B * nh, batch2=nh, a_s1=P * H3, a_s2=hd, b_s1=P * H3, b_s2=hd,
             c_s1=nh * Tp * Tp, c_s2=Tp * Tp)
    _case("qk", d, dict(A=B * P * H3, B=B * P * H3, C=B * nh * Tp * Tp), prec, offs=dict(B=nh * hd), zero_c=True)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_window_segment(prec):
    B, G, Hg, Kt, T, P = 2, 4, 16, 16, 40, 41
    H = G * Hg
    d = dict(M=T, N=Hg, K=Kt * Hg, lda=H, ldb=Kt * Hg, ldc=H, a_kseg=Hg, a_kseg_stride=H, a_window=1, a_pad=Kt // 2,
             a_rows_valid=T, batch=B * G, batch2=G, a_s1=P * H, a_s2=Hg, b_s2=Hg * Kt * Hg, c_s1=P * H, c_s2=Hg,
             bias_s2=Hg, act=1, ld_res=H, res_s1=P * H, res_s2=Hg)
    _case("window", d, dict(A=B * P * H, B=G * Hg * Kt * Hg, C=B * P * H, bias=H, C_pre=B * P * H, residual=B * P * H), prec,
          zero_c=True)


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_gelu_grad_residual_accumulate(prec):
    M, N, K = 140, 96, 64
    _case("gelugrad", dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=2 * N, act=2, ld_aux=2 * N, ld_res=N, accumulate=1),
          dict(A=M * K, B=N * K, C=M * 2 * N, aux=M * 2 * N, residual=M * N), prec, offs=dict(C=N, aux=N))


def _bf_case(name, d, shapes, prec, seed=0, offs=None, x16=False, gate=False):
    """bf16-operand path: A / B are bf16 planes (hi [+ lo]); the reference multiplies exactly those values.
    x16: C_pre / aux are bf16 arrays (aux_bf16 = 1); gate: they hold gelu'(v) (aux_gate = 1)."""
    from paa_amd.model import bf16_bits, bf16_to_f32, split_bf16
    rng = np.random.default_rng(seed)
    host = {k: rng.normal(size=n).astype(np.float32) for k, n in shapes.items()}
    if not d.get("accumulate"):
        host["C"][:] = 0
    bufs, ref = {}, {}
    for k, v in host.items():
        if k in ("A", "B"):
            hi, lo = split_bf16(v)
            bufs[k] = torch.from_numpy(hi.view(np.int16)).cuda()
            bufs[k + "_lo"] = torch.from_numpy(lo.view(np.int16)).cuda()
            ref[k] = (bf16_to_f32(hi).astype(np.float64) + (bf16_to_f32(lo).astype(np.float64) if prec else 0.0))
        elif x16 and k in ("aux", "C_pre"):
            bits = bf16_bits(v)
            bufs[k] = torch.from_numpy(bits.view(np.int16)).cuda()
            ref[k] = bf16_to_f32(bits).astype(np.float64)
        else:
            bufs[k] = dev(v)
            ref[k] = v.astype(np.float64)
    cb = torch.zeros(shapes["C"], dtype=torch.int16, device="cuda")
    cbl = torch.zeros(shapes["C"], dtype=torch.int16, device="cuda")
    bufs["Cb"], bufs["Cb_lo"] = cb, cbl
    dd = dict(d)
    dd.update(precision=prec, operand_bf16=1, aux_bf16=int(x16), aux_gate=int(gate))
    names = {k: k for k in shapes}
    names.update(Cb="Cb")
    if prec:
        names.update(A_lo="A_lo", B_lo="B_lo", Cb_lo="Cb_lo")
    run_gemm({**dd, **names}, bufs, offs)
    o = offs or {}
    de = {k: v for k, v in dd.items() if k not in ("operand_bf16", "aux_bf16")}
    pre_before = ref["C_pre"].copy() if "C_pre" in ref else None
    emulate(de, ref["A"], ref["B"], ref["C"], a_off=o.get("A", 0), b_off=o.get("B", 0), c_off=o.get("C", 0),
            bias=ref.get("bias"), aux=ref.get("aux"), aux_off=o.get("aux", 0), residual=ref.get("residual"),
            res_off=o.get("residual", 0), C_pre=ref.get("C_pre"))
    e = rel_err(bufs["C"].cpu().numpy(), ref["C"])
    got_b = bf16_to_f32(cb.cpu().numpy().view(np.uint16)).astype(np.float64)
    if prec:
        got_b = got_b + bf16_to_f32(cbl.cpu().numpy().view(np.uint16))
    eb = rel_err(got_b, ref["C"])
    ep = 0.0
    if "C_pre" in ref:
        got_p = bufs["C_pre"].cpu().numpy()
        got_p = bf16_to_f32(got_p.view(np.uint16)).astype(np.float64) if x16 else got_p.astype(np.float64)
        ep = rel_err(got_p, ref["C_pre"])
        assert not np.array_equal(ref["C_pre"], pre_before)
    print(f"gemm_bf[{name}] prec={prec} x16={int(x16)} rel_err={e:.3e} bf16-planes rel_err={eb:.3e} C_pre rel_err={ep:.3e}")
    assert e < (3e-5 if prec else 5e-6), name
    assert eb < (3e-5 if prec else 5e-3), name
    # a kept gelu'(v) inherits the product's error scaled by max|v| / max|gelu'| (~30x here)
    assert ep < (5e-3 if x16 else (3e-4 if gate else (3e-5 if prec else 5e-6))), name
    return {k: bufs[k].clone() for k in ("C", "Cb", "Cb_lo", "C_pre") if k in bufs}


@pytest.mark.parametrize("prec", [0, 1])
def test_gemm_bf16_operands(prec):
    M, N, K = 300, 200, 96
    _bf_case("plain", dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, alpha=0.5, act=1), dict(A=M * K, B=N * K, C=M * N, bias=N, C_pre=M * N), prec)
    M, N, K = 257, 384, 1536
    _bf_case("bigk", dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N), dict(A=M * K, B=N * K, C=M * N), prec)
    Cc, k, s, M = 32, 3, 2, 250
    _bf_case("convview", dict(M=M, N=Cc, K=k * Cc, lda=s * Cc, ldb=k * Cc, ldc=Cc, row_period=50, row_valid=49, act=1),
             dict(A=(s * M + 8) * Cc, B=Cc * k * Cc, C=M * Cc, C_pre=M * Cc), prec)
    _bf_case("tallM", dict(M=2500, N=200, K=320, lda=320, ldb=320, ldc=200, act=1), dict(A=2500 * 320, B=200 * 320, C=2500 * 200, bias=200, C_pre=2500 * 200), prec)
    _bf_case("tallM_k64", dict(M=2304, N=384, K=64, lda=64, ldb=64, ldc=384), dict(A=2304 * 64, B=384 * 64, C=2304 * 384), prec)
    _bf_case("n32k40", dict(M=200, N=32, K=40, lda=40, ldb=40, ldc=32), dict(A=200 * 40, B=32 * 40, C=200 * 32, bias=32), prec)
    B, G, Hg, Kt, T, P = 2, 4, 16, 16, 40, 41
    H = G * Hg
    d = dict(M=T, N=Hg, K=Kt * Hg, lda=H, ldb=Kt * Hg, ldc=H, a_kseg=Hg, a_kseg_stride=H, a_window=1, a_pad=Kt // 2,
             a_rows_valid=T, batch=B * G, batch2=G, a_s1=P * H, a_s2=Hg, b_s2=Hg * Kt * Hg, c_s1=P * H, c_s2=Hg,
             bias_s2=Hg, act=1, ld_res=H, res_s1=P * H, res_s2=Hg)
    _bf_case("window", d, dict(A=B * P * H, B=G * Hg * Kt * Hg, C=B * P * H, bias=H, C_pre=B * P * H, residual=B * P * H), prec)
    # grouped positional conv in its slab-kernel form (a_kseg 48 / 64, taps % 4 == 0), forward and dgrad padding
    for Hg, Kt, T, pad in ((48, 8, 150, 4), (48, 16, 300, 7), (48, 8, 100, 3), (48, 128, 499, 64), (64, 8, 131, 4)):
        B, G, P = 2, 2, T + 1
        H = G * Hg
        d = dict(M=T, N=Hg, K=Kt * Hg, lda=H, ldb=Kt * Hg, ldc=H, a_kseg=Hg, a_kseg_stride=H, a_window=1, a_pad=pad,
                 a_rows_valid=T, batch=B * G, batch2=G, a_s1=P * H, a_s2=Hg, b_s2=Hg * Kt * Hg, c_s1=P * H, c_s2=Hg,
                 bias_s2=Hg, act=1, ld_res=H, res_s1=P * H, res_s2=Hg)
        _bf_case(f"slab{Hg}x{Kt}", d, dict(A=B * P * H, B=G * Hg * Kt * Hg, C=B * P * H, bias=H, C_pre=B * P * H, residual=B * P * H), prec)
    # dgrad form: A rows start Q rows back (guard rows), output rows interleaved (ldc = 2 N), gelu' epilogue
    Mr, Co, Ci = 120, 32, 32
    _bf_case("dgrad", dict(M=Mr, N=Ci, K=2 * Co, lda=Co, ldb=2 * Co, ldc=2 * Ci, act=2, ld_aux=2 * Ci),
             dict(A=(Mr + 8) * Co, B=Ci * 2 * Co, C=Mr * 2 * Ci, aux=Mr * 2 * Ci), prec, offs=dict(A=7 * Co, C=Ci, aux=Ci))
    # bf16 storage of the pre-activation (C_pre) and of the GELU-grad operand (aux): vector and scalar epilogues
    _bf_case("tallM_pre16", dict(M=2500, N=200, K=320, lda=320, ldb=320, ldc=200, act=1), dict(A=2500 * 320, B=200 * 320, C=2500 * 200, bias=200, C_pre=2500 * 200), prec, x16=True)
    _bf_case("tallM_aux16", dict(M=2400, N=256, K=128, lda=128, ldb=128, ldc=256, act=2, ld_aux=256), dict(A=2400 * 128, B=256 * 128, C=2400 * 256, aux=2400 * 256), prec, x16=True)
    _bf_case("small_pre16", dict(M=300, N=100, K=96, lda=96, ldb=96, ldc=100, act=1), dict(A=300 * 96, B=100 * 96, C=300 * 100, bias=100, C_pre=300 * 100), prec, x16=True)
    # accumulate into a non-zero C with a residual: vector and scalar epilogues
    _bf_case("tallM_accum", dict(M=2500, N=256, K=128, lda=128, ldb=128, ldc=256, ld_res=256, accumulate=1), dict(A=2500 * 128, B=256 * 128, C=2500 * 256, residual=2500 * 256), prec)
    _bf_case("small_accum", dict(M=300, N=100, K=96, lda=96, ldb=96, ldc=100, ld_res=100, accumulate=1), dict(A=300 * 96, B=100 * 96, C=300 * 100, residual=300 * 100), prec)
    # ... holding gelu'(v) instead of v (aux_gate): vector and scalar epilogues, both directions
    _bf_case("tallM_gate_fwd", dict(M=2500, N=200, K=320, lda=320, ldb=320, ldc=200, act=1), dict(A=2500 * 320, B=200 * 320, C=2500 * 200, bias=200, C_pre=2500 * 200), prec, x16=True, gate=True)
    _bf_case("tallM_gate_bwd", dict(M=2400, N=256, K=128, lda=128, ldb=128, ldc=256, act=2, ld_aux=256), dict(A=2400 * 128, B=256 * 128, C=2400 * 256, aux=2400 * 256), prec, x16=True, gate=True)
    _bf_case("small_gate_fwd", dict(M=300, N=100, K=96, lda=96, ldb=96, ldc=100, act=1), dict(A=300 * 96, B=100 * 96, C=300 * 100, bias=100, C_pre=300 * 100), prec, x16=True, gate=True)
    _bf_case("small_gate_f32", dict(M=300, N=100, K=96, lda=96, ldb=96, ldc=100, act=1), dict(A=300 * 96, B=100 * 96, C=300 * 100, bias=100, C_pre=300 * 100), prec, gate=True)
    _bf_case("dgrad_aux16", dict(M=Mr, N=Ci, K=2 * Co, lda=Co, ldb=2 * Co, ldc=2 * Ci, act=2, ld_aux=2 * Ci),
             dict(A=(Mr + 8) * Co, B=Ci * 2 * Co, C=Mr * 2 * Ci, aux=Mr * 2 * Ci), prec, offs=dict(A=7 * Co, C=Ci, aux=Ci), x16=True)


# the ring configurations of the shipped library; a -DPAA_EXPERIMENTS build (paa_version 301) also holds the measured-and-rejected ones
RING_CFGS = [(0, 8), (1, 7), (1, 20), (0, 21), (1, 22), (0, 23)]
RING_CFGS_EXPERIMENTS = [(0, 2), (0, 3), (0, 5), (0, 12), (0, 14), (0, 15), (1, 4), (1, 6), (1, 11), (1, 13), (1, 16), (1, 17), (1, 18), (0, 19)]


@pytest.mark.parametrize("prec,cfg", RING_CFGS + (RING_CFGS_EXPERIMENTS if os.environ.get("PAA_TEST_EXPERIMENTS") else []))
def test_gemm_ring_configurations(prec, cfg):
    """LDS-DMA ring kernels (csrc/gemm_ring.hip) forced through paa_gemm_config: vs the numpy statement of the descriptor
    and BIT-identical to the register-staged kernel (cfg 1) on the same buffers — M / N edges inside the last tiles, a
    conv-style overlapping A view with a row mask, every epilogue stream of the vector epilogue."""
    L = _lib.lib()
    if (prec, cfg) in RING_CFGS_EXPERIMENTS and L.paa_version() != 301:
        pytest.skip("configuration exists only in -DPAA_EXPERIMENTS builds")
    try:
        for name, d, shapes, kw in [
            ("ring_gelu", dict(M=2200, N=640, K=320, lda=320, ldb=320, ldc=640, alpha=0.5, act=1),
             dict(A=2200 * 320, B=640 * 320, C=2200 * 640, bias=640, C_pre=2200 * 640), dict(x16=prec == 0, gate=prec == 0)),
            ("ring_resid", dict(M=2304, N=768, K=768, lda=768, ldb=768, ldc=768, ld_res=768),
             dict(A=2304 * 768, B=768 * 768, C=2304 * 768, residual=2304 * 768), {}),
            ("ring_convview", dict(M=4000, N=512, K=384, lda=256, ldb=384, ldc=512, row_period=500, row_valid=499, act=2, ld_aux=512),
             dict(A=(2 * 4000 + 8) * 128, B=512 * 384, C=4000 * 512, aux=4000 * 512), dict(x16=prec == 0, gate=prec == 0)),
        ]:
            outs = {}
            for c in (1, cfg):
                L.paa_gemm_config(c)
                outs[c] = _bf_case(f"{name}/cfg{c}", d, shapes, prec, seed=7, **kw)
            for k in outs[1]:
                assert torch.equal(outs[1][k], outs[cfg][k]), (name, k, "ring result differs from the register-staged kernel")
    finally:
        L.paa_gemm_config(0)


@pytest.mark.parametrize("prec,cfg", [(0, 1), (0, 8), (1, 1), (1, 7), (1, 20), (0, 21), (1, 22), (0, 23)])
def test_gemm_k_group_order(prec, cfg):
    """gemm.h k_group: the K slabs of a strided-conv product walked channel-slab-major / tap-minor (3 taps of 128 channels at
    stride 2 here, and the 2-tap window of a stride-2 dgrad) — same products in another f32 summation order, so the
    result is checked against the numpy statement at the usual tolerance, not bit for bit."""
    L = _lib.lib()
    try:
        L.paa_gemm_config(cfg)
        _bf_case(f"kgroup_fwd/cfg{cfg}", dict(M=4000, N=512, K=384, lda=256, ldb=384, ldc=512, row_period=500, row_valid=499, act=1, k_group=128),
                 dict(A=(2 * 4000 + 8) * 128, B=512 * 384, C=4000 * 512, bias=512, C_pre=4000 * 512), prec, seed=11)
        _bf_case(f"kgroup_dgrad/cfg{cfg}", dict(M=4000, N=512, K=512, lda=256, ldb=512, ldc=512, act=2, ld_aux=512, k_group=256),
                 dict(A=(4000 + 8) * 256, B=512 * 512, C=4000 * 512, aux=4000 * 512), prec, seed=12)
    finally:
        L.paa_gemm_config(0)


@pytest.mark.parametrize("cfg", [20, 22])
def test_gemm_interleaved_weight_planes(cfg):
    """paa_gemm_desc.B_il: the weights' hi / lo planes interleaved per 32-element K group (one 128-byte line per K slab of a row).
    Same products in the same order as the planar form, so the results must be bit-identical to it (and it is checked against
    numpy by test_gemm_ring_configurations)."""
    from paa_amd.model import interleave_planes, split_bf16
    L = _lib.lib()
    rng = np.random.default_rng(3)
    M, N, K = 2200, 512, 384
    A, B = rng.normal(size=(M, K)).astype(np.float32), rng.normal(size=(N, K)).astype(np.float32)
    (ah, al), (bh, bl) = split_bf16(A), split_bf16(B)
    t = {k: torch.from_numpy(v.view(np.int16)).cuda() for k, v in dict(ah=ah, al=al, bh=bh, bl=bl, bil=interleave_planes(bh, bl)).items()}
    bias = torch.from_numpy(rng.normal(size=N).astype(np.float32)).cuda()
    outs = []
    try:
        L.paa_gemm_config(cfg)
        for il in (False, True):
            d = _lib.PaaGemmDesc()
            d.A, d.A_lo, d.B, d.B_lo = t["ah"].data_ptr(), t["al"].data_ptr(), t["bh"].data_ptr(), t["bl"].data_ptr()
            d.B_il = t["bil"].data_ptr() if il else None
            d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, K, K, N
            d.a_kcontig = d.b_kcontig = d.batch = d.batch2 = d.operand_bf16 = d.precision = 1
            d.alpha, d.act, d.aux_gate, d.bias = 0.5, 1, 1, bias.data_ptr()
            pre = torch.zeros(M * N, device="cuda"); cb = torch.zeros(M * N, dtype=torch.int16, device="cuda"); cbl = torch.zeros_like(cb)
            d.C_pre, d.Cb, d.Cb_lo = pre.data_ptr(), cb.data_ptr(), cbl.data_ptr()
            _lib.check(L.paa_gemm(C.byref(d), _lib.stream_ptr()))
            torch.cuda.synchronize()
            outs.append((pre.clone(), cb.clone(), cbl.clone()))
    finally:
        L.paa_gemm_config(0)
    assert float(outs[0][0].abs().max()) > 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cfg,case", [(1, "tall"), (20, "tall"), (22, "tall"), (1, "conv"), (20, "conv"), (22, "conv"), (0, "seg_small"), (0, "narrow"), (0, "auto_tall")])
def test_gemm_interleaved_activation_planes(cfg, case):
    """paa_gemm_desc.A_il / Cb_il (fp32-parity mode): the activations' hi / lo planes in ONE array interleaved per 32-element group, as
    operand and as result.  Same products in the same order as the planar form on every kernel that can meet such a tensor — the
    separate-ring kernels (20 / 22), the register-staged ones (1), the general loader (K % 64 != 0) and the narrow tile — so the
    de-interleaved results must equal the planar run bit for bit (which test_gemm_bf16_operands / _ring_configurations check
    against numpy)."""
    from paa_amd.model import split_bf16
    L = _lib.lib()
    rng = np.random.default_rng(5)
    shapes = {  # M, N, K, lda, A elements, extra descriptor fields
        "tall": (2200, 512, 384, 384, 2200 * 384, dict(act=1, aux_gate=1, alpha=0.5)),
        "auto_tall": (16000, 768, 768, 768, 16000 * 768, dict()),
        "conv": (4000, 512, 384, 256, (2 * 4000 + 8) * 128, dict(row_period=500, row_valid=499, act=2, k_group=128)),
        "seg_small": (300, 96, 96, 96, 300 * 96, dict()),
        "narrow": (1000, 32, 768, 768, 1000 * 768, dict()),
    }
    M, N, K, lda, na, extra = shapes[case]
    A = rng.normal(size=na).astype(np.float32)
    Bw = rng.normal(size=(N, K)).astype(np.float32)
    (ah, al), (bh, bl) = split_bf16(A), split_bf16(Bw)
    ail = np.stack([ah.reshape(-1, 32), al.reshape(-1, 32)], axis=1).reshape(-1)           # [32 hi | 32 lo] per group of the flat buffer
    t = {k: torch.from_numpy(v.view(np.int16)).cuda() for k, v in dict(ah=ah, al=al, bh=bh, bl=bl, ail=ail).items()}
    bias = torch.from_numpy(rng.normal(size=N).astype(np.float32)).cuda()
    aux = torch.from_numpy(rng.normal(size=M * N).astype(np.float32)).cuda()
    outs = []
    try:
        L.paa_gemm_config(cfg)
        for il in (False, True):
            d = _lib.PaaGemmDesc()
            d.A, d.A_lo, d.B, d.B_lo = t["ah"].data_ptr(), t["al"].data_ptr(), t["bh"].data_ptr(), t["bl"].data_ptr()
            d.A_il = t["ail"].data_ptr() if il else None
            d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, K, N
            d.a_kcontig = d.b_kcontig = d.batch = d.batch2 = d.operand_bf16 = d.precision = 1
            d.alpha, d.bias = 1.0, bias.data_ptr()
            for k, v in extra.items():
                setattr(d, k, v)
            c32 = torch.zeros(M * N, device="cuda")
            pre = torch.zeros(M * N, device="cuda")
            planes = torch.zeros(2 * M * N, dtype=torch.int16, device="cuda")
            d.C = c32.data_ptr()
            if extra.get("act") == 1:
                d.C_pre = pre.data_ptr()
            if extra.get("act") == 2:
                d.aux, d.ld_aux = aux.data_ptr(), N
            if il and N % 32 == 0:
                d.Cb_il = planes.data_ptr()
            else:
                d.Cb, d.Cb_lo = planes.data_ptr(), planes.data_ptr() + 2 * M * N
            _lib.check(L.paa_gemm(C.byref(d), _lib.stream_ptr()))
            torch.cuda.synchronize()
            pl = planes.cpu().numpy()
            if il and N % 32 == 0:
                g = pl.reshape(-1, 2, 32)
                hi, lo = g[:, 0].reshape(-1), g[:, 1].reshape(-1)
            else:
                hi, lo = pl[:M * N], pl[M * N:]
            outs.append((c32.cpu().numpy().copy(), pre.cpu().numpy().copy(), hi.copy(), lo.copy()))
    finally:
        L.paa_gemm_config(0)
    assert np.abs(outs[0][0]).max() > 0 and np.abs(outs[0][2]).max() > 0
    for name, a, b in zip(("C", "C_pre", "Cb hi", "Cb lo"), *outs):
        assert np.array_equal(a, b), (case, cfg, name)
    # and against a float64 product of the split operands (loose: this is a layout test)
    if case != "conv" and not extra.get("act"):
        ref = (A.reshape(M, K).astype(np.float64) @ Bw.T.astype(np.float64)) + bias.cpu().numpy()
        assert rel_err(outs[1][0].reshape(M, N), ref) < 1e-4


def test_layernorm_fwd_bwd():
    torch.manual_seed(0)
    for rows, cols in ((37, 512), (130, 768), (9, 64), (5, 32)):
        x = torch.randn(rows, cols) * 2 + 0.3
        g = torch.randn(cols) * 0.1 + 1
        b = torch.randn(cols) * 0.1
        dy = torch.randn(rows, cols)
        xr = x.clone().requires_grad_(True)
        yr = F.layer_norm(xr, (cols,), g, b, eps=1e-5)
        yr.backward(dy)
        xd, gd, bd, dyd = x.cuda(), g.cuda(), b.cuda(), dy.cuda()
        y = torch.empty_like(xd); st = torch.empty(rows, 2, device="cuda"); dx = torch.empty_like(xd)
        L = _lib.lib()
        _lib.check(L.paa_layernorm_fwd(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(y), _lib.ptr(st), rows, cols, 1e-5, _lib.stream_ptr()))
        _lib.check(L.paa_layernorm_bwd(_lib.ptr(dyd), _lib.ptr(xd), _lib.ptr(gd), _lib.ptr(st), _lib.ptr(dx), rows, cols, _lib.stream_ptr()))
        torch.cuda.synchronize()
        e1, e2 = rel_err(y.cpu(), yr.detach()), rel_err(dx.cpu(), xr.grad)
        print(f"layernorm {rows}x{cols}: fwd {e1:.2e} bwd {e2:.2e}")
        assert e1 < 1e-5 and e2 < 2e-5


def test_softmax_fwd_bwd():
    torch.manual_seed(1)
    rows, cols, ld = 77, 499, 512
    s = torch.randn(rows, ld) * 3
    dp = torch.randn(rows, ld)
    sr = s[:, :cols].clone().requires_grad_(True)
    pr = torch.softmax(sr * 0.125, -1)
    pr.backward(dp[:, :cols])
    sd, dpd = s.cuda(), dp.cuda()
    L = _lib.lib()
    _lib.check(L.paa_softmax_fwd(_lib.ptr(sd), rows, cols, ld, 0.125, _lib.stream_ptr()))
    _lib.check(L.paa_softmax_bwd(_lib.ptr(dpd), _lib.ptr(sd), rows, cols, ld, 0.125, _lib.stream_ptr()))
    torch.cuda.synchronize()
    e1, e2 = rel_err(sd.cpu()[:, :cols], pr.detach()), rel_err(dpd.cpu()[:, :cols], sr.grad)
    print(f"softmax fwd {e1:.2e} bwd {e2:.2e}")
    assert e1 < 1e-5 and e2 < 2e-5
    assert float(sd[:, cols:].abs().max()) == 0 and float(dpd[:, cols:].abs().max()) == 0


# label capacities: 2 S_max + 1 <= 1024 -> wave-synchronous log-domain kernels (1, 2, 6, 16 states per lane);
# (700, 600): the log-domain kernel for larger capacities; (60, 30, [.., 40->infeasible]) is covered by lens > T below
# (499, 100) and (499, 250): 4 and 8 states per lane — with 2 and 6 the shapes of the one-wave-per-state-slot recursion (k_ctc_rec_mw<NS, 1>);
# (499, 499) and (1499, 450, the 30 s clips): 16 states per lane = sixteen waves of two states (k_ctc_rec_mw<16, 2>)
@pytest.mark.parametrize("T,S_max,lens", [(24, 6, [5, 6, 3, 0]), (499, 150, [150, 120, 1, 77]), (60, 30, [30, 29, 30, 2]),
                                          (80, 40, [40, 1, 33, 40]), (499, 499, [300, 150, 499, 250]), (700, 600, [600, 150, 20, 333]),
                                          (499, 100, [100, 99, 2, 50]), (499, 250, [250, 130, 249, 0]), (1, 40, [1, 0, 1, 1]),
                                          (1499, 450, [450, 301, 1, 449])])
def test_ctc(T, S_max, lens):
    torch.manual_seed(2)
    B, V = len(lens), 32
    logits = torch.randn(B, T, V) * 2
    labels = torch.full((B, S_max), -100, dtype=torch.long)
    for b, n in enumerate(lens):
        labels[b, :n] = torch.randint(1, V, (n,))
        if n > 3:
            labels[b, 2] = labels[b, 1]            # a repeated label forces the blank transition rule
    # float64 torch reference: torch's float32 CPU kernel itself carries ~1e-3 relative noise in the gradient at
    # T=499 (alpha + beta + nll cancels numbers of magnitude 1e3), so the check is against the exact value and the
    # float32 result is only required to be as close to it as torch-float32 is.
    lr = logits.double().clone().requires_grad_(True)
    lp = F.log_softmax(lr, -1).transpose(0, 1)
    mask = labels >= 0
    nll = F.ctc_loss(lp, labels.masked_select(mask), torch.full((B,), T), mask.sum(-1), blank=0, reduction="none",
                     zero_infinity=False)
    nll.sum().backward()
    lg, lab = logits.cuda(), labels.to(torch.int32).cuda()
    out_nll = torch.empty(B, device="cuda"); dl = torch.empty_like(lg)
    L = _lib.lib()
    work = torch.empty(L.paa_ctc_work_floats(B, T, V, S_max), device="cuda")
    _lib.check(L.paa_ctc(_lib.ptr(lg), _lib.ptr(lab), B, T, V, S_max, 0, 1.0, _lib.ptr(out_nll), _lib.ptr(dl), _lib.ptr(work), _lib.stream_ptr()))
    torch.cuda.synchronize()
    fin = torch.isfinite(nll)
    print("ctc nll", out_nll.cpu().tolist(), nll.tolist())
    assert torch.equal(torch.isfinite(out_nll.cpu()), fin)
    e1 = rel_err(out_nll.cpu()[fin], nll.detach()[fin])
    e2 = rel_err(dl.cpu()[fin], lr.grad[fin])
    print(f"ctc T={T}: nll {e1:.2e} grad {e2:.2e}")
    assert e1 < 2e-6 and e2 < 1e-5


# A -inf logit: log-probability -inf must act like any other dead state — zero probability for that class, finite
# loss and gradient wherever the labels avoid it, +inf loss where every alignment needs it — instead of NaN-ing the whole table.
# torch's own backward differentiates through -inf - (-inf); the float64 reference therefore uses -1e4 (probability exp(-1e4) = 0
# in float64 as well) in place of -inf, which is the same function.
def test_ctc_neg_inf_logits():
    torch.manual_seed(9)
    B, T, V, S = 3, 120, 32, 20
    logits = torch.randn(B, T, V) * 2
    logits[:, :, 7] = -float("inf")                      # class 7 impossible everywhere
    logits[0, 10:30, 0] = -float("inf")                  # clip 0: no blank for 20 frames
    labels = torch.full((B, S), -100, dtype=torch.long)
    labels[0, :S] = torch.randint(8, V, (S,))
    labels[1, :12] = torch.randint(8, V, (12,))
    labels[2, :10] = torch.randint(8, V, (10,))
    labels[2, 4] = 7                                     # clip 2 needs the impossible class: loss +inf
    ref_logits = torch.where(torch.isinf(logits), torch.full_like(logits, -1e4), logits)
    lr = ref_logits.double().clone().requires_grad_(True)
    lp = F.log_softmax(lr, -1).transpose(0, 1)
    mask = labels >= 0
    nll = F.ctc_loss(lp, labels.masked_select(mask), torch.full((B,), T), mask.sum(-1), blank=0, reduction="none", zero_infinity=False)
    nll[:2].sum().backward()
    lg, lab = logits.cuda(), labels.to(torch.int32).cuda()
    out_nll = torch.empty(B, device="cuda"); dl = torch.empty_like(lg)
    L = _lib.lib()
    work = torch.empty(L.paa_ctc_work_floats(B, T, V, S), device="cuda")
    _lib.check(L.paa_ctc(_lib.ptr(lg), _lib.ptr(lab), B, T, V, S, 0, 1.0, _lib.ptr(out_nll), _lib.ptr(dl), _lib.ptr(work), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = out_nll.cpu()
    print("ctc -inf logits nll", got.tolist(), nll.tolist())
    assert bool(torch.isfinite(got[:2]).all()) and bool(torch.isinf(got[2])) and float(nll.detach()[2]) > 5e3
    assert bool(torch.isfinite(dl[:2]).all())
    e1, e2 = rel_err(got[:2], nll.detach()[:2]), rel_err(dl.cpu()[:2], lr.grad[:2])
    print(f"ctc -inf logits: nll {e1:.2e} grad {e2:.2e}")
    assert e1 < 2e-6 and e2 < 1e-5
    assert float(dl[:2, :, 7].abs().max()) == 0.0


# Peaked posteriors: a trained CTC model puts the blank far above everything else, and the reference's labels
# are <unk> / | strings, so the target path sits thousands of nats below the all-blank path at every frame.
# A probability-domain recursion rescaled by the row maximum underflows there (loss inf, gradient NaN); the log-domain
# recursion must return the float64 value.  Cases: untargeted-size labels (S=150), the default targeted string
# "delete" x 5 (S=34: all <unk>=3 and |=4), near-uniform control, and 30 s clips (T=1499, lp table read from global).
@pytest.mark.parametrize("T,S,blank_up,unk_down", [(499, 150, 8.0, -15.0), (499, 34, 10.0, -20.0), (499, 150, 3.0, -3.0),
                                                    (1499, 450, 12.0, -25.0), (499, 150, 40.0, -40.0)])
def test_ctc_peaked_logits(T, S, blank_up, unk_down):
    torch.manual_seed(4)
    B, V = 3, 32
    logits = torch.randn(B, T, V) * 0.5
    logits[:, :, 0] += blank_up
    logits[:, :, 3] += unk_down
    labels = torch.full((B, S), -100, dtype=torch.long)
    for b in range(B):
        n = S - 7 * b
        labels[b, :n] = torch.tensor([4 if (i % 6) == 5 else 3 for i in range(n)])      # "uuuuu|uuuuu|..." (F6)
    lr = logits.double().clone().requires_grad_(True)
    lp = F.log_softmax(lr, -1).transpose(0, 1)
    mask = labels >= 0
    nll = F.ctc_loss(lp, labels.masked_select(mask), torch.full((B,), T), mask.sum(-1), blank=0, reduction="none",
                     zero_infinity=False)
    nll.sum().backward()
    assert bool(torch.isfinite(nll).all())
    lg, lab = logits.cuda(), labels.to(torch.int32).cuda()
    out_nll = torch.empty(B, device="cuda"); dl = torch.empty_like(lg)
    L = _lib.lib()
    work = torch.empty(L.paa_ctc_work_floats(B, T, V, S), device="cuda")
    _lib.check(L.paa_ctc(_lib.ptr(lg), _lib.ptr(lab), B, T, V, S, 0, 1.0, _lib.ptr(out_nll), _lib.ptr(dl), _lib.ptr(work), _lib.stream_ptr()))
    torch.cuda.synchronize()
    print("ctc peaked nll", out_nll.cpu().tolist(), nll.tolist())
    assert bool(torch.isfinite(out_nll).all()) and bool(torch.isfinite(dl).all())
    e1 = rel_err(out_nll.cpu(), nll.detach())
    e2 = rel_err(dl.cpu(), lr.grad)
    print(f"ctc peaked T={T} S={S}: nll {e1:.2e} grad {e2:.2e}")
    assert e1 < 2e-6 and e2 < 1e-5


@pytest.mark.parametrize("T,B,nh", [(499, 2, 3), (70, 1, 2), (32, 1, 1), (131, 2, 2)])
def test_fused_attention(T, B, nh):
    """Flash-style attention forward / backward (bf16 operands) vs torch float64 on the same bf16-rounded inputs."""
    from paa_amd.model import bf16_bits, bf16_to_f32
    torch.manual_seed(3)
    hd, P, Tp = 64, T + 1, (T + 31) // 32 * 32
    H = nh * hd
    qkv = (torch.randn(B, P, 3 * H) * 1.5).numpy()
    do = torch.randn(B, P, H).numpy()
    qb, dob = bf16_bits(qkv), bf16_bits(do)
    qr = torch.from_numpy(bf16_to_f32(qb).astype(np.float64)).requires_grad_(True)
    dor = torch.from_numpy(bf16_to_f32(dob).astype(np.float64))
    q, k, v = (qr[:, :T, i * H:(i + 1) * H].reshape(B, T, nh, hd).transpose(1, 2) for i in range(3))
    att = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, -1)
    o = (att @ v).transpose(1, 2).reshape(B, T, H)
    o.backward(dor[:, :T])
    d_qkv = torch.from_numpy(qb.view(np.int16)).cuda()
    d_do = torch.from_numpy(dob.view(np.int16)).cuda()
    ctx = torch.zeros(B, P, H, dtype=torch.int16, device="cuda")
    dqkv = torch.zeros(B, P, 3 * H, dtype=torch.int16, device="cuda")
    lse = torch.zeros(B * nh, Tp, device="cuda")
    delta = torch.zeros(B * nh, Tp, device="cuda")
    L = _lib.lib()
    _lib.check(L.paa_attn_fwd(_lib.ptr(d_qkv), _lib.ptr(ctx), _lib.ptr(lse), B, T, P, Tp, H, nh, _lib.stream_ptr()))
    _lib.check(L.paa_attn_bwd(_lib.ptr(d_qkv), _lib.ptr(ctx), _lib.ptr(lse), _lib.ptr(d_do), _lib.ptr(delta), _lib.ptr(dqkv),
                              B, T, P, Tp, H, nh, _lib.stream_ptr()))
    torch.cuda.synchronize()
    og = bf16_to_f32(ctx.cpu().numpy().view(np.uint16))[:, :T]
    dg = bf16_to_f32(dqkv.cpu().numpy().view(np.uint16))[:, :T]
    e_o = rel_err(og, o.detach().numpy())
    gref = qr.grad.numpy()[:, :T]
    e_q, e_k, e_v = (rel_err(dg[..., i * H:(i + 1) * H], gref[..., i * H:(i + 1) * H]) for i in range(3))
    print(f"attention T={T}: O {e_o:.2e} dQ {e_q:.2e} dK {e_k:.2e} dV {e_v:.2e}")
    assert e_o < 1e-2 and e_q < 2e-2 and e_k < 2e-2 and e_v < 2e-2     # bf16 P / dS and bf16 outputs
    assert float(ctx[:, T:].abs().max()) == 0 and float(dqkv[:, T:].abs().max()) == 0


@pytest.mark.parametrize("T,B,nh", [(499, 2, 3), (70, 1, 2), (131, 2, 2)])
def test_fused_attention_split(T, B, nh):
    """The same kernels with hi + lo planes (split-bf16, fp32-parity mode) vs torch float64 on the f32 inputs."""
    from paa_amd.model import bf16_to_f32, split_bf16
    torch.manual_seed(4)
    hd, P, Tp = 64, T + 1, (T + 31) // 32 * 32
    H = nh * hd
    qkv = (torch.randn(B, P, 3 * H) * 1.5).numpy()
    do = torch.randn(B, P, H).numpy()
    qh, ql = split_bf16(qkv)
    dh, dl = split_bf16(do)
    qv = bf16_to_f32(qh).astype(np.float64) + bf16_to_f32(ql)
    dv = bf16_to_f32(dh).astype(np.float64) + bf16_to_f32(dl)
    qr = torch.from_numpy(qv).requires_grad_(True)
    q, k, v = (qr[:, :T, i * H:(i + 1) * H].reshape(B, T, nh, hd).transpose(1, 2) for i in range(3))
    att = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, -1)
    o = (att @ v).transpose(1, 2).reshape(B, T, H)
    o.backward(torch.from_numpy(dv)[:, :T])
    dev16 = lambda x: torch.from_numpy(x.view(np.int16)).cuda()
    d_qh, d_ql, d_dh, d_dl = dev16(qh), dev16(ql), dev16(dh), dev16(dl)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int16, device="cuda")
    ch, cl, gh, gl = z(B, P, H), z(B, P, H), z(B, P, 3 * H), z(B, P, 3 * H)
    lse = torch.zeros(B * nh, Tp, device="cuda")
    delta = torch.zeros(B * nh, Tp, device="cuda")
    L = _lib.lib()
    _lib.check(L.paa_attn_fwd_split(_lib.ptr(d_qh), _lib.ptr(d_ql), _lib.ptr(ch), _lib.ptr(cl), _lib.ptr(lse), B, T, P, Tp, H, nh,
                                    _lib.stream_ptr()))
    _lib.check(L.paa_attn_bwd_split(_lib.ptr(d_qh), _lib.ptr(d_ql), _lib.ptr(ch), _lib.ptr(cl), _lib.ptr(lse), _lib.ptr(d_dh),
                                    _lib.ptr(d_dl), _lib.ptr(delta), _lib.ptr(gh), _lib.ptr(gl), B, T, P, Tp, H, nh, _lib.stream_ptr()))
    torch.cuda.synchronize()
    planes = lambda hi, lo: bf16_to_f32(hi.cpu().numpy().view(np.uint16)).astype(np.float64) + bf16_to_f32(lo.cpu().numpy().view(np.uint16))
    og, dg = planes(ch, cl)[:, :T], planes(gh, gl)[:, :T]
    e_o = rel_err(og, o.detach().numpy())
    gref = qr.grad.numpy()[:, :T]
    e_q, e_k, e_v = (rel_err(dg[..., i * H:(i + 1) * H], gref[..., i * H:(i + 1) * H]) for i in range(3))
    print(f"split attention T={T}: O {e_o:.2e} dQ {e_q:.2e} dK {e_k:.2e} dV {e_v:.2e}")
    assert e_o < 5e-5 and e_q < 1e-4 and e_k < 1e-4 and e_v < 1e-4
    assert float(ch[:, T:].abs().max()) == 0 and float(gh[:, T:].abs().max()) == 0


def test_spec_pk_primitives(tmp_path):
    """csrc/spec_pk.h: the packed-f32 instructions of the wave FFT are written out with operand modifiers (op_sel / op_sel_hi /
    neg_lo / neg_hi), the first radix-8 exchange as permlane swaps + DPP moves.  tests/hip/spec_pk_test.hip runs every primitive, both
    radix-8 butterflies and the 8 x 8 register/lane transpose on the device against host arithmetic: the modifier semantics are
    checked directly, not only through the projections' goldens."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not on this box")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip", "spec_pk_test.hip")
    exe = str(tmp_path / "spec_pk_test")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-Wno-unused-result", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "transpose_hi: 0 wrong" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]


@pytest.mark.parametrize("cfg,N", [(1, 768), (22, 768), (20, 512), (0, 768), (0, 1024)])
def test_gemm_residual_layernorm_of_stored_input(cfg, N):
    """gemm.h res_ln_stats: the residual the epilogue adds is LayerNorm(x) evaluated from the stored x and its (mean, rstd) rows.
    The 192-row tiles hold the 8 columns' gain / bias in registers, the 256-row tiles re-read them per row group (gemm_dev.h,
    RLN_HELD) — a path the model never takes (its post-LN residual products have N = 768), so it is forced here (cfg 20)."""
    from paa_amd.model import bf16_to_f32, split_bf16
    M, K = 2304, 256
    rng = np.random.default_rng(11)
    A, B = rng.normal(size=(M, K)).astype(np.float32), rng.normal(size=(N, K)).astype(np.float32) * 0.1
    x = rng.normal(size=(M, N)).astype(np.float32) * 2 + 0.3
    g, b = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    mean = x.astype(np.float64).mean(1)
    rstd = 1.0 / np.sqrt(x.astype(np.float64).var(1) + 1e-5)
    stats = np.stack([mean, rstd], 1).astype(np.float32)
    ah, al = split_bf16(A.ravel()); bh, bl = split_bf16(B.ravel())
    Ar = (bf16_to_f32(ah).astype(np.float64) + bf16_to_f32(al)).reshape(M, K)
    Br = (bf16_to_f32(bh).astype(np.float64) + bf16_to_f32(bl)).reshape(N, K)
    ref = Ar @ Br.T + ((x.astype(np.float64) - stats[:, :1].astype(np.float64)) * stats[:, 1:].astype(np.float64)) * g + b
    t = {k: torch.from_numpy(v.view(np.int16)).cuda() for k, v in dict(ah=ah, al=al, bh=bh, bl=bl).items()}
    xd, gd, bd, sd = dev(x.ravel()), dev(g), dev(b), dev(stats.ravel())
    out = torch.zeros(M * N, device="cuda")
    d = _lib.PaaGemmDesc()
    d.a_kcontig = d.b_kcontig = 1
    d.batch = d.batch2 = 1
    d.alpha = 1.0
    d.operand_bf16 = d.precision = 1
    d.A, d.A_lo, d.B, d.B_lo = t["ah"].data_ptr(), t["al"].data_ptr(), t["bh"].data_ptr(), t["bl"].data_ptr()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ld_res = M, N, K, K, K, N, N
    d.C, d.residual = out.data_ptr(), xd.data_ptr()
    d.res_ln_stats, d.res_ln_g, d.res_ln_b = sd.data_ptr(), gd.data_ptr(), bd.data_ptr()
    L = _lib.lib()
    try:
        L.paa_gemm_config(cfg)
        _lib.check(L.paa_gemm(C.byref(d), _lib.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        L.paa_gemm_config(0)
    e = rel_err(out.cpu().numpy().reshape(M, N), ref)
    print(f"res_ln cfg {cfg} N {N}: rel err {e:.2e}")
    assert e < 3e-5
