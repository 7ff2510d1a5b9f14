"""Every C-ABI entry point requires the same pointers, in the same order, and refuses the same arguments with the same
code and message as recorded in tests/golden/abi_requirements.json (tests/abi_corpus.py, tools/gen_abi_requirements.py).

Runs only where no GPU is visible: a call that passes the checks goes on to launch a kernel on dummy pointers, which
must never reach a device.  Without one the launch fails with MD_ELAUNCH, and nothing runs."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_checks_match_fixture():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the corpus calls entry points with dummy pointers")
    import __graft_entry__ as g
    import abi_corpus
    got = abi_corpus.run(g.build_hip())
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_requirements.json")))
    assert sorted(got) == sorted(want)
    bad = ["%s / %s:\n  got  %s\n  want %s" % (e, p, got[e].get(p), want[e].get(p))
           for e in want for p in sorted(set(want[e]) | set(got[e])) if got[e].get(p) != want[e].get(p)]
    assert not bad, "%d (entry, profile) pairs differ:\n%s" % (len(bad), "\n".join(bad[:20]))
