"""TEST INFRASTRUCTURE — writes tests/golden/tier_b_refusals.json from the built library itself: what every int32_t svt_hip_* export
answers to the three probes of tests/test_tier_b_refusals.py in a process that never called svt_hip_init.  The record is the library's
behaviour at the time of writing; regenerate it only when a refusal is meant to change, and read the diff.
    python tests/golden/make_golden_refusals.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "svt-av1-mod-by-patman_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import test_tier_b_refusals as T  # noqa: E402


def main():
    rows = T.census()
    with open(T.GOLD, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(rows[n])}" for n in sorted(rows)) + "\n}\n")
    print(len(rows), "exports ->", T.GOLD, os.path.getsize(T.GOLD), "bytes")


if __name__ == "__main__":
    main()
