"""Writes tests/golden/ctc_rec_parent.json: the bits the wave-synchronous CTC kernels of a commit give on the cases of
tests/test_gpu_rows.py (ws_cases: capacity, full label rows, the wave-synchronous CTC_CASES; both blanks) — nll as uint32 bit
patterns and the SHA-256 of the dlogits bytes.  Run on the GPU with the library built from the commit whose bits are to be kept:

    python tools/ctc_parent_bits.py --commit <hash> [--out tests/golden/ctc_rec_parent.json]

test_ctc_bits_of_the_parent recomputes the same from the same seeds and compares."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ctc_rec_parent.json"))
    a = ap.parse_args()
    import test_gpu_rows as TR
    cases = {}
    for name, (logits, _, _, _) in TR.ws_cases().items():
        V = logits.shape[2]
        cases[name] = {str(blank): TR.ws_bits(name, blank) for blank in (0, V - 1)}
    with open(a.out, "w") as f:
        json.dump({"commit": a.commit, "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")


if __name__ == "__main__":
    main()
