#!/usr/bin/env python3
"""Writes tests/golden/decode_plan_digests.json: the SHA-256 of every descriptor block tests/decode_plan_digests.py plans from the small JPEG and PNG
fixtures.  Host only (the planners need no device).

    python tools/make_decode_plan_digests.py            # writes the file
    python tools/make_decode_plan_digests.py --check    # plans twice, compares with the file, writes nothing

The file is the record of the commit that introduced it: a change to a planner that is meant to keep the block's bytes must leave it unchanged."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decode_plan_digests as G  # noqa: E402


def main():
    got = G.digests()
    if got != G.digests():
        raise SystemExit("two runs gave different digests: the blocks hold bytes the planner did not set")
    if "--check" in sys.argv:
        with open(G.PATH) as f:
            want = json.load(f)
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        print("%d blocks, %d differ from %s" % (len(got), len(bad), os.path.relpath(G.PATH, ROOT)))
        for k in bad[:20]:
            print("  " + k)
        return 1 if bad else 0
    with open(G.PATH, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d blocks -> %s" % (len(got), os.path.relpath(G.PATH, ROOT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
