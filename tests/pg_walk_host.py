"""The host-side form of md_swap_draw's PG walk, applied to an oracle's arrays: the oracle on a PG walk's scene pool
(engine.HostScene with walk_scenarios), stepped with the swap after every step as the engine launches it after md_step.  The schedule is
md_walk_scene of include/md_scenario.h through tests/walk_host.c.  TEST INFRASTRUCTURE."""
import numpy as np

import hostlib
import lane_change_host as lh
import oracle_binding as ob
import walk_host as wh
from metadrive_ped_amd import abi
from metadrive_ped_amd.engine import BatchedEngine

# the live arrays that mirror a pool array (the reset of the respawn modes restores the routes from them)
TWINS = dict(route_nodes="route_nodes0", route_roads="route_roads0", final_lane="final_lane0")


def scene(host, e, ep):
    """md_walk_scene for the host's walk over arrays of (e, ep)"""
    return wh.walk_scene(*host.walk_params, e, ep)


class PgWalkOracle(ob.OracleWorld):
    """An env whose episode has ended moves on to its next scene: scene_of, walk_ep, its own copy of MdWorld.env_map, the rows of
    BatchedEngine.DRAW_ARRAYS from the pool, and the scene's traffic stream (rng) where the batch has one."""

    def __init__(self, host, state=None):
        super().__init__(host, state)
        assert host.walk and host.pool is not None
        self.s.walk = abi.MdWalk(*host.walk_params)
        self.env_map = np.ascontiguousarray(host.world.arrays["env_map"], np.int32).copy()
        self.w.env_map = self.env_map.ctypes.data

    def swap(self):
        h, st, cap = self.host, self.state, self.host.cap
        for e in np.nonzero(st["need_reset"])[0]:
            ep = int(st["walk_ep"][e]) + 1
            p = int(scene(h, e, ep))
            st["walk_ep"][e], st["scene_of"][e], self.env_map[e] = ep, p, p
            rows, prow = slice(e * cap, (e + 1) * cap), slice(p * cap, (p + 1) * cap)
            for k in BatchedEngine.DRAW_ARRAYS:
                st[k][rows] = h.pool[k][prow]
                if k in TWINS and TWINS[k] in st:
                    st[TWINS[k]][rows] = h.pool[k][prow]
            if "rng" in h.pool:
                st["rng"][e] = h.pool["rng"][p]

    def step(self, actions=None, threads=1):
        super().step(actions, threads)
        self.swap()

    def reset(self):
        self.state["walk_ep"][:] = -1
        self.state["need_reset"][:] = 1
        self.swap()
        super().reset()


class PgWalkLaneChangeOracle(lh.LaneChangeOracle):
    """LaneChangeOracle on a walk: the restatement reads the lanes through the oracle's own env_map, which the swap rewrites"""

    def __init__(self, host):
        super().__init__(host)
        k = self.o.k
        self.o = PgWalkOracle(host)
        self.o.k = k

    def step(self, decoded):
        h, st = self.host, self.o.state
        a = h.world.arrays
        act = np.ascontiguousarray(np.asarray(decoded, np.float32).reshape(h.E, h.A, 2)).copy()
        P = hostlib.ptr
        lh.lib().hx_lane_change_batch(P(a["lanes"]), P(a["lane_off"]), P(a["roads"]), P(a["road_off"]), P(self.o.env_map),
                                      P(st["shape"]), P(st["dyn"]), P(st["nav"]), P(st["flags"]), P(st["need_reset"]), P(self.pid),
                                      P(st["pid0"]), P(act), h.E, h.cap, h.A, 0)
        self.o.step(act)
        return act
