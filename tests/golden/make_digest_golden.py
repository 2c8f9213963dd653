#!/usr/bin/env python3
"""Writes tests/golden/digest/traces.json: the per-tick state digests {table, nodes} of the project's CPU
oracle for the cases of tests/digest_cases.py, computed by membership.digest (the NumPy definition of
GM_DIGEST_VERSION 1). Runs the oracle and NumPy only: no GPU, nothing of the reference.

usage: python tests/golden/make_digest_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "distributed-membership_amd"), os.path.join(REPO, "tests")]

import digest_cases  # noqa: E402
from membership import digest  # noqa: E402


def main():
    out = {"version": digest.VERSION, "cases": {name: digest_cases.run(name) for name in digest_cases.CASES}}
    os.makedirs(os.path.dirname(digest_cases.TRACES), exist_ok=True)
    with open(digest_cases.TRACES, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(digest_cases.TRACES, {k: len(v) for k, v in out["cases"].items()})


if __name__ == "__main__":
    main()
