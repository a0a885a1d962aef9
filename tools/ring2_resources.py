"""Code-object resources of every k_gemm_ring2 instantiation, from a cross-compile (no GPU needed):

    python tools/ring2_resources.py [path/to/gemm_ring2.hip]  > profiles/epilogue_kinds_resources.txt

Compiles the file with -Rpass-analysis=kernel-resource-usage -S and prints, per kernel: instructions, branches, v_readlane_b32 (SGPR
spill reloads), global loads / stores (LDS-DMA loads included), VGPRs, spilled SGPRs / VGPRs and scratch bytes.  No instantiation
may use scratch."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "psychoacoustic-adverserial-attacks_amd", "csrc", "gemm_ring2.hip")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wno-unused-value", "--cuda-device-only"] + os.environ.get("PAA_EXTRA_HIPCC_FLAGS", "").split()


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return names
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.split("\n") if r.returncode == 0 else names


def main():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "ring2.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-S", "-c", SRC, "-o", asm], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr)
        res, cur = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"remark:\s+(Function Name|VGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = res.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = int(m.group(2))
        counts, name = {}, None
        for line in open(asm):
            m = re.match(r"^(_Z\w*k_gemm_ring2\w*):", line)
            if m:
                name = m.group(1)
                counts[name] = dict(ins=0, br=0, rl=0, ld=0, st=0)
                continue
            if name is None:
                continue
            t = line.strip()
            if t.startswith("s_endpgm"):
                name = None
                continue
            if not t or t[0] in ".;" or t.endswith(":"):
                continue
            c, op = counts[name], t.split()[0]
            c["ins"] += 1
            c["br"] += op.startswith(("s_cbranch", "s_branch"))
            c["rl"] += op == "v_readlane_b32"
            c["ld"] += op.startswith(("global_load", "buffer_load"))
            c["st"] += op.startswith(("global_store", "buffer_store"))
    names = sorted(counts)
    print(f"{'kernel':92s} {'instr':>6s} {'branch':>6s} {'readlane':>8s} {'ld/st':>9s} {'VGPRs':>5s} {'SGPRspill':>9s} {'VGPRspill':>9s} {'scratch':>7s}")
    bad = 0
    for n, dn in zip(names, demangle(names)):
        c, q = counts[n], res.get(n, {})
        short = re.sub(r"^void paa::\(anonymous namespace\)::|\(paa::GemmArgs\)$|paa::", "", dn)
        print(f"{short:92s} {c['ins']:6d} {c['br']:6d} {c['rl']:8d} {c['ld']:4d}/{c['st']:<4d} {q.get('VGPRs', -1):5d} {q.get('SGPRs Spill', -1):9d} "
              f"{q.get('VGPRs Spill', -1):9d} {q.get('ScratchSize [bytes/lane]', -1):7d}")
        bad += q.get("ScratchSize [bytes/lane]", 0) != 0
    if bad:
        sys.exit(f"{bad} instantiation(s) use scratch")


if __name__ == "__main__":
    main()
