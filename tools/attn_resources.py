"""Code-object resources of the attention backward kernels, from a cross-compile (no GPU needed):

    python tools/attn_resources.py  > profiles/attn_onepass_resources.txt

Compiles csrc/attention.hip with -Rpass-analysis=kernel-resource-usage -S and prints, per backward kernel: VGPRs, AGPRs,
SGPRs (.amdhsa_next_free_sgpr), spilled VGPRs, scratch bytes per lane, static LDS bytes and the instruction count up to s_endpgm.  No kernel may use
scratch."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(HERE, "psychoacoustic-adverserial-attacks_amd", "csrc", "attention.hip")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wno-unused-value", "--cuda-device-only"]
KERNELS = ("k_attn_bwd_dq", "k_attn_bwd_dkv", "k_attn_bwd_one", "k_attn_dq_finish")
FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "SGPRs": "sgpr", "VGPRs Spill": "vspill", "SGPRs Spill": "sspill",
          "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occ"}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    except OSError:
        return names
    return r.stdout.split("\n") if r.returncode == 0 else names


def main():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "attention.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-S", "-c", SRC, "-o", asm],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr)
        res, cur = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = res.setdefault(m.group(2), {})
            elif cur is not None and m.group(1) in FIELDS:
                cur[FIELDS[m.group(1)]] = int(m.group(2))
        counts, name = {}, None
        for line in open(asm):
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
            if m:
                cur = res.setdefault(m.group(1), {})
            m = re.match(r"\s*\.amdhsa_next_free_sgpr (\d+)", line)
            if m and cur is not None:
                cur["sgpr"] = int(m.group(1))
            m = re.match(r"^(_Z\w+):", line)
            if m and any(k in m.group(1) for k in KERNELS):
                name = m.group(1)
                counts[name] = dict(ins=0, mfma=0, lds=0)
                continue
            if name is None:
                continue
            t = line.strip()
            if t.startswith("s_endpgm"):
                name = None
                continue
            if not t or t[0] in ".;" or t.endswith(":"):
                continue
            op = t.split()[0]
            counts[name]["ins"] += 1
            counts[name]["mfma"] += op.startswith("v_mfma")
            counts[name]["lds"] += op.startswith("ds_")
    names = sorted(counts, key=lambda n: (KERNELS.index(next(k for k in KERNELS if k in n)), n))
    print(f"{'kernel':28s} {'VGPRs':>5s} {'AGPRs':>5s} {'SGPRs':>5s} {'VGPRspill':>9s} {'scratch':>7s} {'LDS':>7s} {'waves/SIMD':>10s} {'instr':>6s} "
          f"{'mfma':>5s} {'ds_*':>5s}")
    bad = 0
    for n, dn in zip(names, demangle(names)):
        c, q = counts[n], res.get(n, {})
        short = re.sub(r"^void paa::|\(paa::AttnArgs\)$", "", dn)
        print(f"{short:28s} {q.get('vgpr', -1):5d} {q.get('agpr', -1):5d} {q.get('sgpr', -1):5d} {q.get('vspill', -1):9d} {q.get('scratch', -1):7d} "
              f"{q.get('lds', -1):7d} {q.get('occ', -1):10d} {c['ins']:6d} {c['mfma']:5d} {c['lds']:5d}")
        bad += q.get("scratch", 0) != 0
    if bad:
        sys.exit(f"{bad} kernel(s) use scratch")


if __name__ == "__main__":
    main()
