"""Writes tests/golden/proj_parent.json: one SHA-256 of the output bytes per case of tests/test_gpu_projections.py pin_cases()
(every projection entry, norm, frame geometry and row shape the projection driver decides between).  Run on the GPU with the library
built from the commit whose bits are to be kept:

    python tools/proj_parent_bits.py --commit <hash> [--out tests/golden/proj_parent.json]
    python tools/proj_parent_bits.py --check-only        # the branch assertion alone: the oracle on the CPU, no device

Before it touches the GPU it asserts with the oracle that every statistic of every case lies more than 1e-4 from its projection's
branch, and that each norm with such a branch (l2, linf, snr, tv, fletcher_munson) is rescaled in one case and left alone in another,
under one statistic and under per-row statistics both.  test_projection_bits_of_the_parent recomputes the hashes and compares."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BRANCHING = ("l2", "linf", "snr", "tv", "fletcher_munson")


def check_branches(TP):
    seen = set()
    for name, case in TP.pin_cases().items():
        form = "universal" if case[4] in ("all", "low") else "rows"
        for moved, dist in TP.pin_branches(case):
            assert dist > 1e-4, ("a statistic on its projection's branch", name, dist)
            if moved is not None:
                seen.add((case[0], form, moved))
    for norm in BRANCHING:
        for form in ("universal", "rows"):
            assert (norm, form, True) in seen and (norm, form, False) in seen, (norm, form, sorted(seen))
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "proj_parent.json"))
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    import test_gpu_projections as TP
    seen = check_branches(TP)
    print(f"branches: {len(seen)} (norm, form, rescaled?) combinations, every statistic more than 1e-4 from its branch")
    if a.check_only:
        return
    if not a.commit:
        ap.error("--commit is required to write the fixture")
    cases = {name: TP.pin_sha256(case) for name, case in TP.pin_cases().items()}
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")


if __name__ == "__main__":
    main()
