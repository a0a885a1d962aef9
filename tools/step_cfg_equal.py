"""Is one fp32-parity step (base architecture, B = 2, L = 16000) the same under forced GEMM configurations?  Run on the GPU box:

    python tools/step_cfg_equal.py                                               # shipped library
    PAA_EXTRA_HIPCC_FLAGS=-DPAA_EXPERIMENTS python tools/step_cfg_equal.py       # diagnostic library: also kinds on / off

Prints, per configuration (20, 22, automatic), whether logits and gradient equal those of configuration 1 bit for bit, and the
largest difference; with the diagnostic library also each configuration with the epilogue kinds against itself under PAA_NO_EPIK=1."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from paa_amd import _lib, arch as A, synth
from paa_amd.model import PaaModel


def main():
    a, B, L = A.BASE, 2, 16000
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L, seed=5)).cuda()
    p = (torch.from_numpy(synth.perturbation(L, seed=5)) * np.float32(2e-3)).cuda()
    labels = torch.tensor([[3, 7, 4, 9, 5], [6, 4, 11, -1, -1]], dtype=torch.int32, device="cuda")
    lib = _lib.lib()
    print(f"library version {lib.paa_version()}")

    def step(cfg, no_epik=False):
        os.environ["PAA_NO_EPIK"] = "1" if no_epik else "0"
        lib.paa_gemm_config(cfg)
        r = m.fwd_bwd(clean, p, labels)
        torch.cuda.synchronize()
        lib.paa_gemm_config(0)
        return r["grad"].clone(), r["logits"].clone()

    def cmp(name, x, ref):
        (g, lg), (g1, l1) = x, ref
        print(f"{name}: logits equal {torch.equal(lg, l1)} max|diff| {float((lg - l1).abs().max()):.3e} of {float(l1.abs().max()):.3e} | "
              f"grad equal {torch.equal(g, g1)} max|diff| {float((g - g1).abs().max()):.3e} of {float(g1.abs().max()):.3e}", flush=True)

    ref = step(1)
    outs = {c: step(c) for c in (20, 22, 0)}
    for c in (20, 22, 0):
        cmp(f"cfg {c} vs cfg 1", outs[c], ref)
    cmp("cfg 20 vs cfg 22", outs[20], outs[22])
    if lib.paa_version() == 351:
        for c in (20, 22):
            cmp(f"cfg {c}: kinds vs PAA_NO_EPIK=1", outs[c], step(c, no_epik=True))


if __name__ == "__main__":
    main()
