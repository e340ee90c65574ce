#!/usr/bin/env python3
"""Record what every workload of tests/batcher_trace.py makes a tree's ContinuousBatcher ask of its engine — every call with its
arguments, and every result dict without its clock readings — against the recording fake engine (no GPU).
tests/golden/batcher_trace_parent.json is this record of the commit BEFORE each per-request feature was gathered into one object
in continuous.py; tests/test_batcher_trace_host.py holds the batcher to it.

    python scripts/record_batcher_trace.py --out trace.json                                  # this tree
    python scripts/record_batcher_trace.py --tree /elsewhere/checkout --commit b14e3fa --out tests/golden/batcher_trace_parent.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose teal_amd package is recorded (default: this one)")
    ap.add_argument("--commit", default="", help="commit id of the recorded tree, kept in the record")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))  # (the workloads are this tree's, whichever package they drive)
    import batcher_trace as T
    names = list(T.workloads())
    with open(args.out, "w") as f:  # one workload per line: a diff of two records names the workload
        f.write('{"commit": %s, "workloads": {\n' % json.dumps(args.commit))
        f.write(",\n".join(f"{json.dumps(n)}: {json.dumps(T.record(n), separators=(',', ':'))}" for n in names))
        f.write("\n}}\n")
    print(f"[record] {len(names)} workloads of {os.path.abspath(args.tree)} -> {args.out} ({os.path.getsize(args.out)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
