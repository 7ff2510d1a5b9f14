"""Host builds of single headers for the CPU tests: build(stem) compiles tests/<stem>.c once per process with the oracle's flags
(COMMON of oracle/Makefile, plus -O2) into one temporary directory that is removed at exit.  TEST INFRASTRUCTURE."""
import atexit
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIBS = {}
_DIR = []


def common_flags():
    """COMMON of oracle/Makefile, its -I../include made absolute"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        common = re.search(r"^COMMON\s*=\s*(.*)$", fh.read(), re.M).group(1).split()
    return [f for f in common if not f.startswith("-I")] + ["-I" + os.path.join(ROOT, "include")]


def build(stem, declare=None):
    """-> ctypes.CDLL of tests/<stem>.c; declare(lib) sets its argtypes, once"""
    if stem not in _LIBS:
        if not _DIR:
            _DIR.append(tempfile.mkdtemp(prefix="md_hostlib_"))
            atexit.register(shutil.rmtree, _DIR[0], ignore_errors=True)
        out = os.path.join(_DIR[0], "lib{}.so".format(stem))
        subprocess.check_call(["gcc", "-O2"] + common_flags() + ["-shared", os.path.join(ROOT, "tests", stem + ".c"), "-o", out, "-lm"])
        _LIBS[stem] = C.CDLL(out)
        if declare is not None:
            declare(_LIBS[stem])
    return _LIBS[stem]


def ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def lane_index(host, state, e=0, a=0):
    """current_lane.index[-1] of agent a of env e (MdLane.idx of MdNav.lane), -1 without a lane"""
    lane = int(state["nav"]["lane"][e * host.cap + a])
    if lane < 0:
        return -1
    arr = host.world.arrays
    m = int(arr["env_map"][e])
    return int(arr["lanes"][int(arr["lane_off"][m]) + lane]["idx"])
