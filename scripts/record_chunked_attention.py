#!/usr/bin/env python3
"""Record what every case of tests/chunked_attention_cases.py leaves — sha256 of the yt bits (all slots) and of the written K / V
cache rows — from a build of the library, as real launches of teal_verify_attention, teal_batched_decode_attention and
teal_batched_decode_attention_slots on the GPU of this machine.  tests/golden/chunked_attention_parent.json is this record of the
commit BEFORE the two attention kernels were folded into teal_chunked_attention.h; tests/test_chunked_attention_gpu.py holds the
kernels to it.

    python scripts/record_chunked_attention.py --out chunked_attention.json                      # the build in the tree
    TEAL_LIB_PATH=/elsewhere/libteal_hip.so python scripts/record_chunked_attention.py \\
        --commit 1e1783f --out tests/golden/chunked_attention_parent.json
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
    ap.add_argument("--commit", default="", help="commit id of the recorded build, kept in the record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import chunked_attention_cases as C
    from teal_amd import _lib, runtime
    L = _lib.load()  # (TEAL_LIB_PATH: another build)
    runtime.init()
    num_cu = L.teal_init()
    assert num_cu > 0, "no GPU"
    cases = {}
    for heads, dtype in C.GROUPS:
        cases.update(C.run_group(L, heads, dtype, runtime.stream_ptr()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "num_cu": num_cu, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"[record] {len(cases)} cases on {num_cu} CUs -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
