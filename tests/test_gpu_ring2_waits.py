"""-m gpu: the separate-ring GEMM (csrc/gemm_ring2.hip) after its waits were re-counted — operand DMA as MUBUF buffer loads, the
counted wait through the builtin, epilogue vectors fetched unconditionally from clamped addresses and settled where first used
(csrc/gemm_dev.h).  None of that may change a bit: every field pattern the model's fp32-parity products use,
forced onto configurations 20 (256 x 256) and 22 (192 x 256), is compared BIT FOR BIT — f32 result, both planes (planar and
interleaved), the kept gate — against configuration 1 (register-staged kernels) and against the same configuration without the
weights' interleaved copy (the generic epilogue on the same main loop).

Shapes, the smallest at which the changed code can go wrong:
  * M = N = 320: ragged last tiles in both directions — the clamped rows of the operand DMA and of the epilogue's lookahead loads, lanes
    outside the matrix that now read (and must not write);
  * K = 96 and K = 160: three and five 32-element slabs — both rings wrap, the `ahead` and the `!ahead` form of the counted wait run;
  * more tiles than the device has CUs (K = 96): workgroups run an epilogue FOLLOWED by another tile's K loop — the boundary where a
    load the compiler still took for pending used to drain the next loop; two back-to-back launches must give equal bits.

One detail carried over from tests/test_gpu_epilogue_kinds.py (its docstring): at K % 64 != 0 configuration 1 takes its scalar epilogue,
whose GELU goes through libm's erff, so the GELU-FORWARD patterns are compared bit for bit to configuration 1 at K = 192 (six slabs)
and at K = 96 / 160 bit for bit to the generic ring epilogue; every other pattern holds against configuration 1 at K = 96 / 160.
Against the diagnostic library (-DPAA_EXPERIMENTS) every kind is taken, and each case asserts through paa_debug_last_epilogue_kind
that the classifier named it.  The shipped library holds GELU_FWD, GELU_GRAD and PLANES: against it the resid and resid_ln patterns run
the generic epilogue, so the folded RESID / RESID_LN code (and the lookahead forms of GELU_GRAD) is covered by a diagnostic build only:

    PAA_EXTRA_HIPCC_FLAGS=-DPAA_EXPERIMENTS python psychoacoustic-adverserial-attacks_amd/build_ext.py
    PAA_EXTRA_HIPCC_FLAGS=-DPAA_EXPERIMENTS python -m pytest -m gpu tests/test_gpu_ring2_waits.py"""
import pytest
import torch

from test_gpu_epilogue_kinds import KIND_ID, Case, TILE_ROWS, _same

pytestmark = pytest.mark.gpu

#            id                    kind         Case arguments
PATTERNS = [("gelu_fwd_bias",     "gelu_fwd",  dict(ail=True, bias=True, mask=True)),
            ("gelu_fwd_nobias",   "gelu_fwd",  dict(ail=True, bias=False)),
            ("gelu_grad_f32gate", "gelu_grad", dict(ail=True)),
            ("planes_bias",       "planes",    dict(ail=True, bias=True)),
            ("planes_nobias",     "planes",    dict(ail=True, bias=False)),
            ("resid",             "resid",     dict(ail=True)),
            ("resid_ln",          "resid_ln",  dict(ail=False))]
IDS = [p[0] for p in PATTERNS]


@pytest.fixture(autouse=True)
def _every_kind_taken(monkeypatch):
    """diagnostic library: every kind taken per launch; the shipped library reads neither variable"""
    monkeypatch.setenv("PAA_EPIK_MASK", "255")
    monkeypatch.delenv("PAA_NO_EPIK", raising=False)


def _bits(case, cfg, against_cfg1):
    got = case.run(cfg)
    if case.took is not None:          # diagnostic library: the classifier gave the pattern its kind (bias-free GELU forward included), not GENERIC
        assert case.took == KIND_ID[case.kind], (case.kind, case.took)
    assert any(bool(v.any()) for v in got.values())
    _same(got, case.run(cfg, bil=False), f"cfg {cfg} vs the generic ring epilogue (no B_il)")
    if against_cfg1:
        _same(got, case.run(1), f"cfg {cfg} vs configuration 1")
    return got


@pytest.mark.parametrize("cfg", [20, 22])
@pytest.mark.parametrize("name,kind,kw", PATTERNS, ids=IDS)
def test_small_ragged(name, kind, kw, cfg):
    """320 x 320, K = 96 and 160 (GELU forward: also K = 192, where configuration 1 is a bit-for-bit reference)"""
    for K in (96, 160) + ((192,) if kind == "gelu_fwd" else ()):
        c = Case(kind, 320, 320, K, seed=31 + K, want_ref=False, **kw)
        _bits(c, cfg, against_cfg1=kind != "gelu_fwd" or K % 64 == 0)


@pytest.mark.parametrize("cfg", [20, 22])
@pytest.mark.parametrize("name,kind,kw", PATTERNS, ids=IDS)
def test_more_tiles_than_cus(name, kind, kw, cfg):
    """an epilogue followed by another tile's K loop in the same workgroup; twice in a row, equal bits"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = cus // 2 + 2
    M, N, K = TILE_ROWS[cfg] * rows, 512, 96
    assert rows * (N // 256) > cus
    c = Case(kind, M, N, K, seed=41, want_ref=False, **kw)
    first = _bits(c, cfg, against_cfg1=kind != "gelu_fwd")
    _same(first, c.run(cfg), f"cfg {cfg}: second launch")
    if kind == "gelu_fwd":          # K = 192 (six slabs): configuration 1's vector epilogue, an independent bit-for-bit reference at this shape too
        _bits(Case(kind, M, N, 192, seed=42, want_ref=False, **kw), cfg, against_cfg1=True)
