"""-m gpu: the epilogue KINDS of the separate-ring GEMM (csrc/gemm_dev.h EPK_*, csrc/gemm_ring2.hip): every kind's descriptor as
csrc/model.hip builds it in fp32-parity mode, forced onto configurations 20 (256 x 256) / 22 (192 x 256), must give what
configuration 1 (the register-staged kernels, generic epilogue) gives, bit for bit, and the numpy statement of the descriptor within
the split-bf16 tolerance.  Each kind is reached only with the weights' interleaved copy (B_il); the same run WITHOUT it takes the
generic epilogue on the same main loop, so `no B_il` is a second bit-for-bit reference on every case.  The shipped library holds and
takes the GELU_FWD kind only (the one that pays); the others exist in -DPAA_EXPERIMENTS builds, and against the
shipped library their cases check the classifier's plumbing, the generic ring epilogue at these shapes and the forced configurations
below the automatic selection's floor.
To run the file against the diagnostic library, where the kinds exist:

    PAA_EXTRA_HIPCC_FLAGS=-DPAA_EXPERIMENTS python psychoacoustic-adverserial-attacks_amd/build_ext.py
    PAA_EXTRA_HIPCC_FLAGS=-DPAA_EXPERIMENTS python -m pytest tests/test_gpu_epilogue_kinds.py

(paa_amd/_lib.py loads libpaa_hip_exp.so under that variable.)  There every case also asserts, through paa_debug_last_epilogue_kind, that
the classifier gave the kind the case names — GENERIC for every near-miss — and the whole step is compared, kinds on against
PAA_NO_EPIK=1, bit for bit under configurations 20 and 22.

One shape detail: at K = 160 (five 32-element slabs, odd, so both operand rings wrap inside and across tiles) configuration 1 runs
its general loader (K % 64 != 0) whose scalar epilogue evaluates GELU through libm's erff, while every vector epilogue, generic or
not, takes the 1.5e-7 erf of paa_common.h.  For the GELU-forward kind the bit-for-bit comparison to configuration 1 is therefore made
at K = 320 (ten slabs: configuration 1's vector epilogue), and K = 160 is compared bit for bit to the generic ring epilogue and to
configuration 1 at the numpy tolerance.  Every other kind holds bit for bit against configuration 1 at K = 160 too."""
import ctypes as C

import numpy as np
import pytest
import torch

from gemm_ref import emulate
from gpu_util import dev, rel_err
from paa_amd import _lib

pytestmark = pytest.mark.gpu
TILE_ROWS = {20: 256, 22: 192}
TOL = 3e-5           # split-bf16 products against float64 (tests/test_gpu_kernels.py, _bf_case)
TOL_GATE = 3e-4      # a kept gelu'(v): the product's error scaled by max|v| / max|gelu'|  (same place)


@pytest.fixture(autouse=True)
def _every_kind_taken(monkeypatch):
    """Diagnostic library: every kind is taken while a test of this file runs (PAA_EPIK_MASK, read per launch) and the generic-epilogue
    switch is off; both are put back afterwards.  The shipped library reads neither."""
    monkeypatch.setenv("PAA_EPIK_MASK", "255")
    monkeypatch.delenv("PAA_NO_EPIK", raising=False)


def _planes(x):
    from paa_amd.model import split_bf16
    hi, lo = split_bf16(np.ascontiguousarray(x, dtype=np.float32).ravel())
    return hi, lo


def _il(hi, lo):
    """flat planes -> one array interleaved per 32-element group (gemm.h A_il / Cb_il)"""
    return np.ascontiguousarray(np.stack([hi.reshape(-1, 32), lo.reshape(-1, 32)], axis=1).reshape(-1))


def _unil(a):
    g = a.reshape(-1, 2, 32)
    return g[:, 0].reshape(-1), g[:, 1].reshape(-1)


class Case:
    """Operands of one product, built once; run(cfg, ...) fills a fresh descriptor and fresh outputs."""

    def __init__(self, kind, M, N, K, seed, lda=None, a_off=0, a_rows=None, ail=False, dgrad=False, cil=True, mask=False, bias=None,
                 want_ref=True):
        from paa_amd.model import bf16_to_f32, interleave_planes
        self.kind, self.M, self.N, self.K, self.ail, self.cil, self.mask = kind, M, N, K, ail, cil, mask
        self.lda = lda or K
        self.a_off = a_off
        self.ldc = 2 * N if dgrad else N              # dgrad addressing: this residue class owns columns N .. 2N of rows of 2N
        self.c_off = N if dgrad else 0
        rng = np.random.default_rng(seed)
        na = (a_rows or M) * self.lda
        A = rng.normal(size=na).astype(np.float32)
        Bw = rng.normal(size=(N, K)).astype(np.float32) * np.float32(1.0 / np.sqrt(K))
        ah, al = _planes(A)
        bh, bl = _planes(Bw)
        self.t = {k: torch.from_numpy(v.view(np.int16)).cuda() for k, v in
                  dict(ah=ah, al=al, bh=bh, bl=bl, ail=_il(ah, al), bil=interleave_planes(bh.reshape(N, K), bl.reshape(N, K))).items()}
        self.has_bias = bias if bias is not None else kind in ("gelu_fwd", "resid_ln")
        self.rng = rng
        self.h = dict(bias=rng.normal(size=N).astype(np.float32), g=rng.normal(size=N).astype(np.float32), b=rng.normal(size=N).astype(np.float32))
        if kind == "gelu_grad":
            self.h["aux"] = rng.normal(size=M * self.ldc).astype(np.float32)
        if kind in ("resid", "resid_ln"):
            self.h["res"] = rng.normal(size=M * N).astype(np.float32)
        self.d = {k: dev(v) for k, v in self.h.items()}
        if kind == "resid_ln":        # statistics as the model has them: from the LayerNorm kernel
            self.stats = torch.zeros(2 * M, device="cuda")
            y = torch.zeros(M * N, device="cuda")
            _lib.check(_lib.lib().paa_layernorm_fwd(_lib.ptr(self.d["res"]), _lib.ptr(self.d["g"]), _lib.ptr(self.d["b"]), _lib.ptr(y),
                                                    _lib.ptr(self.stats), M, N, 1e-5, _lib.stream_ptr()))
            torch.cuda.synchronize()
        self.Ar = None
        if want_ref:
            self.Ar = bf16_to_f32(ah).astype(np.float64) + bf16_to_f32(al)
            self.Br = (bf16_to_f32(bh).astype(np.float64) + bf16_to_f32(bl)).reshape(-1)

    def fields(self, **change):
        """descriptor fields of the kind as csrc/model.hip sets them (+ the near-miss changes of the exactness tests)"""
        f = dict(alpha=1.0, accumulate=0, x16=False, extra_bias=False)
        f.update(change)
        return f

    def run(self, cfg, bil=True, **change):
        f = self.fields(**change)
        M, N, K, t, k = self.M, self.N, self.K, self.t, self.kind
        if f["accumulate"] and "c0" not in self.h:
            self.h["c0"] = self.rng.normal(size=M * self.ldc).astype(np.float32)
            self.d["c0"] = dev(self.h["c0"])
        if f["x16"] and k == "gelu_grad" and not hasattr(self, "aux16"):
            self.aux16 = torch.from_numpy(_planes(self.h["aux"])[0].view(np.int16)).cuda()
        d = _lib.PaaGemmDesc()
        d.a_kcontig = d.b_kcontig = d.batch = d.batch2 = d.operand_bf16 = d.precision = 1
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, self.lda, K, self.ldc
        d.alpha, d.accumulate = f["alpha"], f["accumulate"]
        d.A, d.A_lo = t["ah"].data_ptr() + 2 * self.a_off, t["al"].data_ptr() + 2 * self.a_off
        if self.ail:
            d.A_il = t["ail"].data_ptr() + 4 * self.a_off
        d.B, d.B_lo = t["bh"].data_ptr(), t["bl"].data_ptr()
        d.B_il = t["bil"].data_ptr() if bil else None
        out = {}
        n_out = M * self.ldc
        if self.has_bias or f["extra_bias"]:
            d.bias = self.d["bias"].data_ptr()
        want_c = k in ("resid", "resid_ln") or f["accumulate"]
        if want_c:
            out["C"] = self.d["c0"].clone() if f["accumulate"] else torch.zeros(n_out, device="cuda")
            d.C = out["C"].data_ptr() + 4 * self.c_off
        if k in ("gelu_fwd", "gelu_grad", "planes"):
            out["planes"] = torch.zeros(2 * n_out, dtype=torch.int16, device="cuda")
            if self.cil and k != "planes":
                d.Cb_il = out["planes"].data_ptr() + 4 * self.c_off
            else:
                d.Cb, d.Cb_lo = out["planes"].data_ptr() + 2 * self.c_off, out["planes"].data_ptr() + 2 * (n_out + self.c_off)
        if k == "gelu_fwd":
            d.act, d.aux_gate, d.aux_bf16 = 1, 1, int(f["x16"])
            out["C_pre"] = torch.zeros(n_out, dtype=torch.int16 if f["x16"] else torch.float32, device="cuda")
            d.C_pre = out["C_pre"].data_ptr()
            if self.mask:
                d.row_period, d.row_valid = 100, 99
        if k == "gelu_grad":
            d.act, d.aux_gate, d.aux_bf16, d.ld_aux = 2, 1, int(f["x16"]), self.ldc
            d.aux = (self.aux16.data_ptr() + 2 * self.c_off) if f["x16"] else (self.d["aux"].data_ptr() + 4 * self.c_off)
        if k in ("resid", "resid_ln"):
            d.residual, d.ld_res = self.d["res"].data_ptr(), N
        if k == "resid_ln":
            d.res_ln_stats, d.res_ln_g, d.res_ln_b = self.stats.data_ptr(), self.d["g"].data_ptr(), self.d["b"].data_ptr()
        L = _lib.lib()
        try:
            L.paa_gemm_config(cfg)
            _lib.check(L.paa_gemm(C.byref(d), _lib.stream_ptr()))
            torch.cuda.synchronize()
            self.took = L.paa_debug_last_epilogue_kind() if L.paa_version() == 351 else None      # diagnostic library only
        finally:
            L.paa_gemm_config(0)
        return out

    def result(self, out):
        """the product as (M, N) float64 from whatever the kind writes"""
        from paa_amd.model import bf16_to_f32
        M, N = self.M, self.N
        if "planes" in out:
            pl = out["planes"].cpu().numpy().view(np.uint16)
            hi, lo = _unil(pl) if (self.cil and self.kind != "planes") else (pl[:M * self.ldc], pl[M * self.ldc:])
            v = bf16_to_f32(hi).astype(np.float64) + bf16_to_f32(lo)
        else:
            v = out["C"].cpu().numpy().astype(np.float64)
        return v.reshape(M, self.ldc)[:, self.c_off:self.c_off + N]

    def numpy(self, **change):
        """(C, C_pre) of tests/gemm_ref.py's statement of the descriptor"""
        f = self.fields(**change)
        M, N, K, k = self.M, self.N, self.K, self.kind
        dd = dict(M=M, N=N, K=K, lda=self.lda, ldb=K, ldc=self.ldc, alpha=f["alpha"], accumulate=f["accumulate"],
                  act={"gelu_fwd": 1, "gelu_grad": 2}.get(k, 0), aux_gate=int(k in ("gelu_fwd", "gelu_grad")), ld_aux=self.ldc, ld_res=N)
        if k == "gelu_fwd" and self.mask:
            dd.update(row_period=100, row_valid=99)
        Cr = self.h["c0"].astype(np.float64) if f["accumulate"] else np.zeros(M * self.ldc)
        pre = np.zeros(M * self.ldc) if k == "gelu_fwd" else None
        res = None
        if k == "resid":
            res = self.h["res"].astype(np.float64)
        if k == "resid_ln":
            st = self.stats.cpu().numpy().astype(np.float64).reshape(M, 2)
            res = (((self.h["res"].astype(np.float64).reshape(M, N) - st[:, :1]) * st[:, 1:]) * self.h["g"] + self.h["b"]).reshape(-1)
        emulate(dd, self.Ar, self.Br, Cr, a_off=self.a_off, c_off=self.c_off,
                bias=self.h["bias"].astype(np.float64) if (self.has_bias or f["extra_bias"]) else None,
                aux=self.h["aux"].astype(np.float64) if k == "gelu_grad" else None, aux_off=self.c_off, residual=res, C_pre=pre)
        return Cr.reshape(M, self.ldc)[:, self.c_off:self.c_off + N], None if pre is None else pre.reshape(M, N)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


KIND_ID = dict(generic=0, gelu_fwd=1, gelu_grad=2, resid=3, resid_ln=4, planes=5)      # csrc/gemm_dev.h EPK_*


def _check(case, cfg, against_cfg1=True, **change):
    got = case.run(cfg, **change)
    if case.took is not None:         # a changed field must send the descriptor to the generic epilogue, an unchanged one to its kind
        assert case.took == KIND_ID["generic" if change else case.kind], (case.kind, change, case.took)
    assert float(np.abs(case.result(got)).max()) > 0
    _same(got, case.run(cfg, bil=False, **change), f"cfg {cfg}: kind vs the generic ring epilogue (no B_il)")
    ref1 = case.run(1, **change)
    if against_cfg1:
        _same(got, ref1, f"cfg {cfg} vs configuration 1")
    if case.Ar is not None:
        Cn, pre = case.numpy(**change)
        for name, o in (("kind", got), ("cfg1", ref1)):
            e = rel_err(case.result(o), Cn)
            print(f"{case.kind} cfg {cfg} [{name}] rel_err {e:.3e}")
            assert e < TOL, (case.kind, name)
            if pre is not None and o["C_pre"].dtype == torch.float32:
                ep = rel_err(o["C_pre"].cpu().numpy().reshape(case.M, case.N), pre)
                print(f"{case.kind} cfg {cfg} [{name}] C_pre rel_err {ep:.3e}")
                assert ep < TOL_GATE, (case.kind, name, "C_pre")
    return got


def _shape(cfg):
    return 2 * TILE_ROWS[cfg] + 88, 640, 160       # ragged last row tile | two full column tiles + a 128-column one | five K slabs


@pytest.mark.parametrize("cfg", [20, 22])
@pytest.mark.parametrize("mask", [False, True])
def test_gelu_fwd(cfg, mask):
    """bias + GELU, f32 gate to C_pre, interleaved planes out; with the row mask the dead rows are zero in planes and gate.
    K = 160: bit for bit against the generic ring epilogue, tolerance against configuration 1 (its scalar epilogue there has libm's
    erff, module docstring); K = 320: bit for bit against configuration 1."""
    M, N, K = _shape(cfg)
    for k, exact1 in ((K, False), (2 * K, True)):
        c = Case("gelu_fwd", M, N, k, seed=21, ail=True, mask=mask)
        got = _check(c, cfg, against_cfg1=exact1)
        if mask:
            dead = (np.arange(M) % 100) >= 99
            assert dead.sum() >= 4
            assert not c.result(got)[dead].any() and not got["C_pre"].cpu().numpy().reshape(M, N)[dead].any()
            assert c.result(got)[~dead].any(axis=1).all()


@pytest.mark.parametrize("cfg", [20, 22])
@pytest.mark.parametrize("variant", ["plain_il", "dgrad_il", "dgrad_planar"])
def test_gelu_grad(cfg, variant):
    """acc x f32 gate, planes out.  dgrad: ldc = ld_aux = 2N at element offset N, and A rows that start Q = 4 rows back behind guard
    rows (K = 5 rows of 32 channels); interleaved and planar planes."""
    M, N, K = _shape(cfg)
    if variant == "plain_il":
        c = Case("gelu_grad", M, N, K, seed=22)
    else:
        c = Case("gelu_grad", M, N, K, seed=23, lda=32, a_off=7 * 32, a_rows=M + 16, ail=True, dgrad=True, cil=variant == "dgrad_il")
    got = _check(c, cfg)
    if variant != "plain_il":          # the other residue class's columns stay untouched
        pl = got["planes"].cpu().numpy()
        hi, lo = _unil(pl) if c.cil else (pl[:M * 2 * N], pl[M * 2 * N:])
        assert not hi.reshape(M, 2 * N)[:, :N].any() and not lo.reshape(M, 2 * N)[:, :N].any()


@pytest.mark.parametrize("ail", [False, True])
def test_resid(ail):
    M, N, K = _shape(22)
    _check(Case("resid", M, N, K, seed=24, ail=ail), 22)


@pytest.mark.parametrize("ail", [False, True])
def test_resid_ln(ail):
    """f32 C = acc + bias + LN(stored x), N = 768, statistics from paa_layernorm_fwd"""
    M, _, K = _shape(22)
    _check(Case("resid_ln", M, 768, K, seed=25, ail=ail), 22)


@pytest.mark.parametrize("bias", [False, True])
def test_planes(bias):
    M, N, K = _shape(22)
    _check(Case("planes", M, N, K, seed=26, ail=True, bias=bias), 22)


NEAR_MISSES = [("gelu_fwd", 20, dict(alpha=0.5)), ("gelu_fwd", 22, dict(x16=True)), ("gelu_fwd", 22, dict(accumulate=1)),
               ("gelu_grad", 20, dict(alpha=0.5)), ("gelu_grad", 22, dict(extra_bias=True)), ("gelu_grad", 20, dict(x16=True)),
               ("gelu_grad", 22, dict(accumulate=1)),
               ("resid", 22, dict(alpha=0.5)), ("resid", 22, dict(accumulate=1)), ("resid", 22, dict(extra_bias=True)),
               ("resid_ln", 22, dict(alpha=0.5)), ("resid_ln", 22, dict(accumulate=1)),
               ("planes", 22, dict(alpha=0.5)), ("planes", 22, dict(accumulate=1))]


@pytest.mark.parametrize("kind,cfg,change", NEAR_MISSES, ids=[f"{k}-{c}-{'-'.join(ch)}" for k, c, ch in NEAR_MISSES])
def test_classifier_exactness(kind, cfg, change):
    """A kind's descriptor with ONE field changed must not take the kind's folded path: still configuration 1 bit for bit (K = 320:
    configuration 1's vector epilogue, module docstring), and the numpy statement of the CHANGED descriptor.  (accumulate starts from
    a non-zero C; where the kind has no f32 result the change adds one, as accumulate needs it.)"""
    M, N, _ = _shape(cfg)
    c = Case(kind, M, 768 if kind == "resid_ln" else N, 320, seed=27, ail=kind != "resid")
    if change.get("x16"):               # a bf16 gate is outside gemm_ref's statement of the f32 one: bit-equality only
        c.Ar = None
    _check(c, cfg, **change)


@pytest.mark.parametrize("cfg", [20, 22])
@pytest.mark.parametrize("kind", ["gelu_grad", "resid"])
def test_workgroup_walks_several_tiles(cfg, kind):
    """More tiles than CUs: workgroups go round the persistent tile loop, the rings carry on across the tile boundary"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = TILE_ROWS[cfg] * (cus // 2 + 4), 512, 96
    assert (M // TILE_ROWS[cfg]) * (N // 256) > cus
    c = Case(kind, M, N, K, seed=28, ail=True, want_ref=False)
    _check(c, cfg)


def test_whole_step(monkeypatch):
    """Base architecture, B = 2, L = 16000, fp32 mode: gradient and logits under configurations 20, 22, the automatic selection and 1.

    * automatic selection == configuration 1, bit for bit.
    * 20 == 22, bit for bit: both walk K in 32-element slabs, so every product sums in the same order, while 20 holds only the two
      GELU kinds and 22 all five — the f32-result and plane kinds of 22 against the generic epilogue of 20 on a whole step.
    * 20 / 22 against configuration 1: NOT bit for bit, before this change either — measured on the commit before the kinds, same
      inputs (profiles/epilogue_kinds_step_cfg.txt, tools/step_cfg_equal.py): logits max |diff| 3.0e-5, gradient 2.6e-4 of 14.6.
      The strided-conv products carry gemm.h's k_group order, which
      interleaves the taps per K slab of the KERNEL (32 elements in the rings, 64 in the register-staged kernels): another f32
      summation order, as gemm.h says (tests/test_gpu_kernels.py::test_gemm_k_group_order checks it at a tolerance for the same
      reason).  They are held to the fp32-parity tolerances of tests/test_gpu_model.py (activations 3e-4, gradients 2e-3 of max|ref|).
    """
    from paa_amd import arch as A, synth
    from paa_amd.model import PaaModel
    a, B, L = A.BASE, 2, 16000
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    p = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
    labels = torch.tensor([[3, 7, 4, 9, 5], [6, 4, 11, -1, -1]], dtype=torch.int32, device="cuda")
    lib, outs = _lib.lib(), {}
    try:
        for cfg in (1, 20, 22, 0):
            lib.paa_gemm_config(cfg)
            r = m.fwd_bwd(clean, p, labels)
            torch.cuda.synchronize()
            outs[cfg] = (r["grad"].clone(), r["logits"].clone())
    finally:
        lib.paa_gemm_config(0)
    if lib.paa_version() == 351:      # diagnostic library: what the kinds must not change — the same configuration under the generic epilogue
        monkeypatch.setenv("PAA_NO_EPIK", "1")
        try:
            for cfg in (20, 22):
                lib.paa_gemm_config(cfg)
                r = m.fwd_bwd(clean, p, labels)
                torch.cuda.synchronize()
                assert torch.equal(r["grad"], outs[cfg][0]) and torch.equal(r["logits"], outs[cfg][1]), f"cfg {cfg}: kinds differ from PAA_NO_EPIK=1"
        finally:
            monkeypatch.delenv("PAA_NO_EPIK")
            lib.paa_gemm_config(0)
    g1, l1 = outs[1]
    assert float(g1.abs().max()) > 0 and bool(torch.isfinite(l1).all()) and bool(torch.isfinite(g1).all())
    assert torch.equal(outs[0][0], g1) and torch.equal(outs[0][1], l1), "automatic selection differs from configuration 1"
    assert torch.equal(outs[20][0], outs[22][0]), "grad: configuration 20 differs from 22"
    assert torch.equal(outs[20][1], outs[22][1]), "logits: configuration 20 differs from 22"
    for cfg in (20, 22):
        e_g, e_l = rel_err(outs[cfg][0].cpu().numpy(), g1.cpu().numpy()), rel_err(outs[cfg][1].cpu().numpy(), l1.cpu().numpy())
        print(f"whole step cfg {cfg} vs 1: grad rel_err {e_g:.3e} logits rel_err {e_l:.3e}")
        assert e_l < 3e-4 and e_g < 2e-3, cfg
