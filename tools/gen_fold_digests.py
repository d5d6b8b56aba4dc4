#!/usr/bin/env python3
"""Records the exact bits of the floating folds for tests/golden/fold_digests.json (needs the GPU; tests/test_gpu_fold_digests.py reads
the JSON and recomputes).  The cases are tests/fold_digest_cases.py's, run through aquery2_amd's public Python API alone, so that the
same file runs at any commit that has aqg_rangew, aqg_grouped_rangew and aqg_interval_fold.

    python tools/gen_fold_digests.py         # rewrites tests/golden/fold_digests.json

The digests pin the BRACKETING of the floating sums: run this only in a change that alters the order of combination on purpose."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "fold_digests.json")

ABOUT = ("sha256[:16] (tests/golden_util.py digest) of the outputs of aqg_rangew, aqg_grouped_rangew and aqg_interval_fold, SUM and AVG over "
         "float32 / float64 columns, by case of tests/fold_digest_cases.py; made on an MI355X by tools/gen_fold_digests.py.  The digests pin "
         "the bracketing of the floating sums (which operands of the block tree are combined in which order): they are regenerated only "
         "by a change that alters the bracketing on purpose, never to make a refactor pass.")


def main():
    import aquery2_amd
    import fold_digest_cases
    dev = aquery2_amd.Device(0)
    got = fold_digest_cases.outputs(dev)
    dev.close()
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        json.dump({"about": ABOUT, "digests": {k: d for k, (d, _) in got.items()}}, f, indent=0)
        f.write("\n")
    print(out, len(got), "digests")


if __name__ == "__main__":
    main()
