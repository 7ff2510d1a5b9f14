#!/usr/bin/env python
"""Record tests/golden/abi_requirements.json: what every C-ABI entry point requires and refuses (tests/abi_corpus.py).

    python tools/gen_abi_requirements.py LIBMDSTEP_SO [OUT_JSON]

LIBMDSTEP_SO is the library whose behaviour the fixture pins: to record a refactor's baseline, build its parent commit
(for example in a `git worktree` outside this tree) and pass that library.  Only on a machine without a GPU: a call
that passes the checks would launch a kernel on dummy pointers.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import abi_corpus  # noqa: E402


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    if torch.cuda.device_count() > 0:
        sys.exit("a GPU is visible: the corpus runs only on machines without one")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "abi_requirements.json")
    res = abi_corpus.run(os.path.abspath(sys.argv[1]))
    with open(out, "w") as f:
        f.write(abi_corpus.dumps(res))
    print("%s: %d entry points, %d (entry, profile) pairs" % (out, len(res), sum(len(v) for v in res.values())))


if __name__ == "__main__":
    main()
