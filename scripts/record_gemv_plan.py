#!/usr/bin/env python3
"""Record what every case of tests/gemv_plan_cases.py gets from a build of the library — return code, *nslabs_out and the launch
description — as real launches on the GPU of this machine.  tests/golden/gemv_plan_parent.json is this record of the commit
BEFORE the launch plan was gathered in teal_gemv_plan.h; tests/test_gemv_plan_host.py and tests/test_gemv_plan_gpu.py hold the
plan to it.

    python scripts/record_gemv_plan.py --out gemv_plan.json                      # the build in the tree
    TEAL_LIB_PATH=/elsewhere/libteal_hip.so python scripts/record_gemv_plan.py \\
        --diag-lib /elsewhere/libteal_hip_diag.so --commit 151c3b4 --out tests/golden/gemv_plan_parent.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--diag-lib", default=None, help="the diagnostics build to record (default: the tree's)")
    ap.add_argument("--commit", default="", help="commit id of the recorded build, kept in the record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import gemv_plan_cases as C
    from teal_amd import _lib
    L = _lib.load()  # (TEAL_LIB_PATH: another build)
    D = _lib._open(args.diag_lib, True) if args.diag_lib else _lib.load_diag()
    num_cu = L.teal_init()
    assert num_cu > 0 and D.teal_init() == num_cu, "no GPU"
    got_fused, got_legacy = C.run_table(L, D)
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "num_cu": num_cu, "fused": got_fused, "legacy": got_legacy}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"[record] {len(got_fused)} fused + {len(got_legacy)} legacy cases on {num_cu} CUs -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
