"""ctypes binding of tests/walk_host.c (md_walk_scene of include/md_scenario.h, compiled by tests/hostlib.py)
and the host-side form of md_swap_draw's scenario walk, applied to an oracle's arrays.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
import oracle_binding as ob
from metadrive_ped_amd import abi
from metadrive_ped_amd.scenario import walk_params



def _declare(L):
    P = C.c_void_p
    L.hx_walk_scene.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, P, P, C.c_int, P]


def lib():
    return hostlib.build("walk_host", _declare)


def walk_scene(n_scenes, walk, stride, offset, seed, e, ep):
    """md_walk_scene over arrays of (e, ep)"""
    e, ep = np.broadcast_arrays(np.asarray(e, np.int32), np.asarray(ep, np.int32))
    shape = e.shape
    e, ep = np.ascontiguousarray(e, np.int32).ravel(), np.ascontiguousarray(ep, np.int32).ravel()
    out = np.zeros(e.shape, np.int32)
    lib().hx_walk_scene(n_scenes, walk, stride, offset, seed, e.ctypes.data, ep.ctypes.data, e.size, out.ctypes.data)
    return out.reshape(shape)


def cfg_walk_scene(cfg, e, ep):
    return walk_scene(*walk_params(cfg), e, ep)


class WalkOracle(ob.OracleWorld):
    """The oracle on a walk's scene pool, stepped with the host-side form of md_swap_draw after every step (as the engine
    launches it after md_step): an env whose episode has ended moves on to its next scene -- scene_of, walk_ep, its own copy of
    MdWorld.env_map, and the snapshot rows from the pool."""
    ROWS = ("shape0", "dyn0", "nav0", "pid0", "param")

    def __init__(self, host, state=None):
        super().__init__(host, state)
        self.set_tracks(host.tracks["shape"], host.tracks["dyn"])
        self.s.walk = abi.MdWalk(*host.walk_params)
        self.env_map = np.ascontiguousarray(host.world.arrays["env_map"], np.int32).copy()
        self.w.env_map = self.env_map.ctypes.data

    def swap(self):
        h, st, cap = self.host, self.state, self.host.cap
        for e in np.nonzero(st["need_reset"])[0]:
            ep = int(st["walk_ep"][e]) + 1
            p = int(cfg_walk_scene(h.cfg, e, ep))
            st["walk_ep"][e], st["scene_of"][e], self.env_map[e] = ep, p, p
            for k in self.ROWS:
                st[k][e * cap:(e + 1) * cap] = h.pool[k][p * cap:(p + 1) * cap]

    def step(self, actions=None, threads=1):
        super().step(actions, threads)
        self.swap()

    def reset(self):
        self.state["walk_ep"][:] = -1
        self.state["need_reset"][:] = 1
        self.swap()
        super().reset()
