"""Where every k_gemm_ring2 instantiation waits for vector memory, from a cross-compile (no GPU needed):

    python tools/ring2_waits.py [--label NAME] [--asm shipped.s experiments.s]  >> profiles/ring2_waits.txt

Compiles csrc/gemm_ring2.hip twice (the shipped flags, and -DPAA_EXPERIMENTS) to assembly and prints one row per kernel:

  K loop   every `s_waitcnt` with a vmcnt(N) field inside the K loop, as N, in text order.  The kernel's own certifying wait is the
           one a barrier follows with no MFMA or memory operation between: it shows as the pair `0 GA` (the `!ahead` and the `ahead`
           form, one of which runs) once per copy of the slab's end.  Any OTHER wait is the compiler's, carries a `!`, and sits on
           the slab path or on a cursor's move to the next tile.
  foreign  how many K-loop waits carry a `!`;  drains: how many of those are vmcnt(0), each a drain of the operand pipeline.  Must be 0.
  epi v0   vmcnt(0) waits after the last K loop in text order (the epilogue, and the prologue's out-of-line blocks).
  epi st   epilogue waits that wait FOR A STORE: the epilogue is walked in text order with a queue of its loads and stores (vmcnt
           retires in issue order); a wait whose youngest retired operation is a store asks for more than any load needs.  Branches
           are not followed — the count is exact for the straight-line epilogues of the folded kinds and a rough reading for the
           generic one, whose loads sit behind run-time tests.  Must be 0 for the folded kinds of the SHIPPED build.  The kinds only the
           diagnostic build holds are listed, not judged: EpiResid / EpiResidLn wait at the top of a row group, i.e. also for the
           previous group's stores (the early wait was measured on them and lost), and EpiGeluGradAhead<N> are
           A/B controls that keep that placement on purpose (N = 1: the form GELU_GRAD had before).
  ld/st    global loads (LDS-DMA loads included) / stores of the whole kernel;  VGPRs, scratch bytes per lane from the listing.

The K loop is found from the listing alone: basic blocks from labels and branches, natural loops from back edges, and a loop counts as
a K loop when it holds MFMAs and no smaller MFMA loop inside it.  Exit status 1 if any kernel has a foreign wait in its K loop, or a
folded kind (anything but EpiGeneric) of the shipped build an epi st."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(HERE, "psychoacoustic-adverserial-attacks_amd", "csrc")
SRC = os.path.join(CSRC, "gemm_ring2.hip")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wno-unused-value", "--offload-device-only", "-S"]
BUILDS = [("shipped", []), ("experiments", ["-DPAA_EXPERIMENTS"])]


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    except OSError:
        return names
    return r.stdout.split("\n") if r.returncode == 0 else names


def functions(path):
    """-> {mangled name: (instruction lines, trailer comment lines)}"""
    out, name, body = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w*k_gemm_ring2\w*):", line)
        if m:
            name, body = m.group(1), []
            out[name] = (body, [])
            continue
        if name is None:
            continue
        t = line.strip()
        if body is not None:
            if t.startswith(".Lfunc_end"):
                body = None
            else:
                t = t.split(";")[0].strip()
                if t and not (t[0] == "." and not t.endswith(":")):
                    body.append(t)
        else:
            if t.startswith(("; NumVgprs:", "; ScratchSize:")):
                out[name][1].append(t)
            if t.startswith(".type") or t.startswith(".text"):
                name = None
    return out


def vm_n(t):
    """N of an s_waitcnt's vmcnt field, or None"""
    if not t.startswith("s_waitcnt"):
        return None
    m = re.search(r"vmcnt\((\d+)\)", t)
    if m:
        return int(m.group(1))
    m = re.match(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)\s*$", t)       # raw immediate: vmcnt = bits 3:0 and 15:14 (gfx9)
    if m:
        v = int(m.group(1), 0)
        n = (v & 0xF) | ((v >> 14) & 0x3) << 4
        return None if n == 63 else n
    return None


def is_load(op):
    return op.startswith(("global_load", "buffer_load", "flat_load", "scratch_load"))


def is_store(op):
    return op.startswith(("global_store", "buffer_store", "flat_store", "scratch_store", "global_atomic", "buffer_atomic", "flat_atomic"))


def blocks_of(body):
    """basic blocks: list of (first, last + 1) instruction indices, successor lists, labels -> block"""
    leaders, labels = {0}, {}
    for i, t in enumerate(body):
        if t.endswith(":"):
            leaders.add(i)
            labels[t[:-1]] = i
        elif t.split()[0].startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            leaders.add(i + 1)
    starts = sorted(x for x in leaders if x < len(body))
    bidx = {}
    blocks = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(body)
        blocks.append((s, e))
        bidx[s] = k
    succ = [[] for _ in blocks]
    for k, (s, e) in enumerate(blocks):
        last = next((body[i] for i in range(e - 1, s - 1, -1) if not body[i].endswith(":")), "")
        op = last.split()[0] if last else ""
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = last.split()[-1]
            if tgt in labels:
                succ[k].append(bidx[labels[tgt]])
        if not op.startswith(("s_branch", "s_endpgm", "s_setpc")) and k + 1 < len(blocks):
            succ[k].append(k + 1)
    return blocks, succ


def dominators(succ, n):
    pred = [[] for _ in range(n)]
    for a, ss in enumerate(succ):
        for b in ss:
            pred[b].append(a)
    full = (1 << n) - 1
    dom = [full] * n
    dom[0] = 1
    changed = True
    while changed:
        changed = False
        for b in range(1, n):
            d = full
            for p in pred[b]:
                d &= dom[p]
            d |= 1 << b
            if d != dom[b]:
                dom[b], changed = d, True
    return dom, pred


def natural_loops(succ, dom, pred):
    """header -> set of blocks (loops sharing a header merged) and its latches"""
    loops = {}
    for a, ss in enumerate(succ):
        for h in ss:
            if dom[a] >> h & 1:          # back edge a -> h
                body, work = loops.setdefault(h, ({h}, []))
                work.append(a)
                stack = [a]
                while stack:
                    x = stack.pop()
                    if x not in body:
                        body.add(x)
                        stack.extend(pred[x])
    return loops


def certifies(body, blocks, succ, b, i, depth=4):
    """the wait at instruction i of block b reaches a barrier before any MFMA, LDS or memory operation (through the few branches of
    the two-form diamond)"""
    for t in body[i + 1:blocks[b][1]]:
        if t.endswith(":"):
            continue
        op = t.split()[0]
        if op == "s_barrier":
            return True
        if op.startswith(("v_mfma", "ds_")) or is_load(op) or is_store(op):
            return False
    return depth > 0 and any(certifies(body, blocks, succ, nb, blocks[nb][0] - 1, depth - 1) for nb in succ[b])


def analyse(body):
    blocks, succ = blocks_of(body)
    n = len(blocks)
    dom, pred = dominators(succ, n)
    loops = natural_loops(succ, dom, pred)
    has_mfma = [any(body[i].startswith("v_mfma") for i in range(s, e)) for s, e in blocks]
    mfma_loops = {h: v for h, v in loops.items() if any(has_mfma[b] for b in v[0])}
    kloops = [h for h, v in mfma_loops.items()
              if not any(h2 != h and v2[0] < v[0] for h2, v2 in mfma_loops.items())]
    res = dict(loops=[], drain=0, foreign=0)
    last_end = 0
    for h in sorted(kloops):
        lb, latches = mfma_loops[h]
        waits = []
        for b in sorted(lb):
            s, e = blocks[b]
            last_end = max(last_end, e)
            for i in range(s, e):
                w = vm_n(body[i])
                if w is not None:
                    own = certifies(body, blocks, succ, b, i)
                    waits.append(f"{w}{'' if own else '!'}")
                    res["foreign"] += not own
                    res["drain"] += (not own) and w == 0
        res["loops"].append(waits)
    # epilogue: text after the last K-loop block; queue of loads (L) / stores (S) in issue order
    q, v0, st = [], 0, 0
    for t in body[last_end:]:
        if t.endswith(":"):
            continue
        op = t.split()[0]
        if is_load(op):
            q.append("L")
        elif is_store(op):
            q.append("S")
        else:
            w = vm_n(t)
            if w is None:
                continue
            v0 += w == 0
            retired, q = (q[:len(q) - w], q[len(q) - w:]) if w < len(q) else ([], q)
            st += bool(retired) and retired[-1] == "S"
    res["epi_v0"], res["epi_st"] = v0, st
    ops = [t.split()[0] for t in body if not t.endswith(":")]
    res["ld"], res["st"] = sum(map(is_load, ops)), sum(map(is_store, ops))
    res["v0"] = sum(vm_n(t) == 0 for t in body)
    return res


def compile_asm(extra, out):
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-I", os.path.join(HERE, "include"), SRC, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--asm", nargs=2, metavar=("SHIPPED.s", "EXPERIMENTS.s"), help="read these listings instead of compiling")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if a.asm:
            paths = a.asm
        else:
            with ThreadPoolExecutor(max_workers=2) as ex:
                paths = list(ex.map(lambda b: compile_asm(b[1], os.path.join(tmp, b[0] + ".s")), BUILDS))
        bad = 0
        for (bname, _), path in zip(BUILDS, paths):
            fns = functions(path)
            names = sorted(fns)
            print(f"== {a.label + ': ' if a.label else ''}{bname} build ==")
            print(f"{'kernel':64s} {'K loop vmcnt(N)  (! = not its own)':40s} {'foreign':>7s} {'drains':>6s} {'epi v0':>6s} {'epi st':>6s} {'all v0':>6s} {'ld/st':>9s} {'VGPRs':>5s} {'scratch':>7s}")
            for nme, dn in zip(names, demangle(names)):
                body, trailer = fns[nme]
                r = analyse(body)
                short = re.sub(r"^void paa::\(anonymous namespace\)::k_gemm_ring2|\(paa::GemmArgs\)$|paa::", "", dn)
                vg = next((int(t.split(":")[1]) for t in trailer if "NumVgprs" in t), -1)
                sc = next((int(t.split(":")[1]) for t in trailer if "ScratchSize" in t), -1)
                kl = " | ".join(" ".join(w) for w in r["loops"]) or "(no loop found)"
                print(f"{short:64s} {kl:40s} {r['foreign']:7d} {r['drain']:6d} {r['epi_v0']:6d} {r['epi_st']:6d} {r['v0']:6d} {r['ld']:4d}/{r['st']:<4d} {vg:5d} {sc:7d}")
                bad += (r["foreign"] != 0) + (r["epi_st"] != 0 and "EpiGeneric" not in short and bname == "shipped") + (not r["loops"])
            print()
    if bad:
        sys.exit(f"{bad} finding(s): a wait in a K loop that is not the kernel's own, a shipped folded kind whose epilogue waits for a store, or no K loop found")


if __name__ == "__main__":
    main()
