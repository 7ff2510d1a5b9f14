"""Host builds of single headers for the CPU tests: build(stem) compiles tests/<stem>.c once per process with the oracle's flags
(COMMON of oracle/Makefile, plus -O2) into one temporary directory that is removed at exit.  And what the *_host.py modules of the
side features share: HostRows (per-env row blocks in host memory), the structs over a host scene or a hand-built world, put / clear.
TEST INFRASTRUCTURE."""
import atexit
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from metadrive_ped_amd import abi

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


class HostRows:
    """The rows [E, row bytes] of one (table, row bytes) pair of abi.row_blocks, in host memory"""
    def __init__(self, table, row_bytes, E):
        self.table, self.rows = table, np.zeros((E, row_bytes), np.uint8)

    def ptrs(self):
        """name -> address of env 0's block, for the blocks that have bytes"""
        return abi.block_ptrs(self.table, self.rows.ctypes.data)

    def out(self, name):
        """a typed copy of the block `name`, [E, ...]"""
        return abi.block_of(self.rows, self.table, name)

    def outs(self):
        return {name: self.out(name) for name in self.table}

    def set(self, name, value):
        off, _, dt = self.table[name]
        self.rows[:, off:off + abi.block_bytes(self.table, name)] = np.ascontiguousarray(value, dt).reshape(len(self.rows), -1).view(np.uint8)


def structs_of(host, state, env_map=None):
    """(MdWorld, MdState, MdConfig, keep-alive) over the host scene's tables and the numpy state `state` (the oracle's, or one
    downloaded from the device); env_map: the envs' maps when they are not the scene's own (a walking batch)"""
    from metadrive_ped_amd.engine import make_structs
    wa = dict(host.world.arrays, **host.world_scalars())
    if env_map is not None:
        wa["env_map"] = np.ascontiguousarray(env_map, np.int32)
    state = {k: np.ascontiguousarray(v) for k, v in state.items()}
    w, s, k = make_structs(wa, state, host.md_config, host.world.n_maps, host.E, ptr)
    return w, s, k, (wa, state)


def hand_built_structs(world, state, **config):
    """(MdWorld, MdState, MdConfig) of a hand-built world of ONE map: `world` the MdWorld arrays and scalars by field, `state` the
    MdState arrays, `config` the MdConfig fields beyond struct_size, n_envs = 1 and agents_per_env = 1.  The structs hold bare
    addresses: the two dicts ride along as keep_alive."""
    k = abi.MdConfig()
    k.struct_size, k.n_envs, k.agents_per_env = C.sizeof(abi.MdConfig), 1, 1
    for f, v in config.items():
        setattr(k, f, v)
    w = abi.MdWorld()
    w.n_maps, w.n_envs = 1, k.n_envs
    for f, v in world.items():
        setattr(w, f, ptr(v) if isinstance(v, np.ndarray) else v)
    s = abi.MdState()
    for f, v in state.items():
        setattr(s, f, ptr(v))
    w.keep_alive, s.keep_alive = world, state
    return w, s, k


def put(st, slot, x, y, heading=0.0, kind=abi.KIND_VEHICLE, flags=abi.F_ALIVE, hl=2.25, hw=0.9, speed=0.0):
    """a mover into a slot of a hand-built state"""
    sh = st["shape"][slot]
    sh["cx"], sh["cy"], sh["c"], sh["s"], sh["hl"], sh["hw"] = x, y, math.cos(heading), math.sin(heading), hl, hw
    sh["flags"], sh["aux"] = kind | flags, -1
    st["dyn"][slot]["heading"], st["dyn"][slot]["speed"] = heading, speed


def clear(st, slot):
    st["shape"][slot]["flags"] = 0


def lane_index(host, state, e=0, a=0):
    """current_lane.index[-1] of agent a of env e (MdLane.idx of MdNav.lane), -1 without a lane"""
    lane = int(state["nav"]["lane"][e * host.cap + a])
    if lane < 0:
        return -1
    arr = host.world.arrays
    m = int(arr["env_map"][e])
    return int(arr["lanes"][int(arr["lane_off"][m]) + lane]["idx"])
