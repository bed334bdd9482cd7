#!/usr/bin/env python3
"""The recording tests/test_gpu_pool_replay.py replays: every case of that file played once on
the MI355X, by the build of the commit whose behaviour is to be pinned.

Run it twice and compare the files before committing one: a case that differs between two
runs of the same build is not a recording.

Usage: python tests/golden/gen_golden_pools.py [output file]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import test_gpu_pool_replay as replay  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "pool_replay.json")
    with open(out, "w") as fh:
        json.dump({name: replay.play(name) for name in replay.CASES}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(replay.CASES)} cases -> {out}")


if __name__ == "__main__":
    main()
