"""ctypes binding of tests/lane_change_host.c, the host build of include/md_lane_change.h (compiled on first use into a
temporary directory by tests/hostlib.py), and the CPU oracle driven by it: LaneChangePolicy's reference run
without a GPU.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
from hostlib import lane_index, ptr as _p      # noqa: F401  (lane_index: the tests read it from here)

PID_ERRS = ("hp", "hi", "hd", "lp", "li", "ld")     # the lane-change PIDs' state in an MdPid row


def _declare(L):
    P, i, f = C.c_void_p, C.c_int, C.c_float
    L.hx_target.argtypes = [P, P, i, i, i]
    L.hx_target.restype = i
    L.hx_steer.argtypes = [P, f, f, f, P]
    L.hx_steer.restype = f
    L.hx_lane_change_batch.argtypes = [P] * 13 + [i, i, i, i]
    L.hx_lane_change_batch.restype = None


def lib():
    return hostlib.build("lane_change_host", _declare)


def target(lanes, roads, cur, road0, direction):
    return lib().hx_target(_p(lanes), _p(roads), cur, road0, direction)


def steer(lane, x, y, heading, pid):
    """md_lane_change_steer on one lane record; pid: a PID_DT row array of length 1, updated in place"""
    lane = np.ascontiguousarray(np.asarray(lane).reshape(1))
    return float(lib().hx_steer(_p(lane), x, y, heading, _p(pid)))


class LaneChangeOracle:
    """The CPU oracle stepped with LaneChangePolicy's actions from the host restatement.  The oracle runs the host's config
    with agent_idm = 0 (EnvInputPolicy): it cannot run the policy, and would take agent_idm != 0 for IDMPolicy.  self.pid
    holds the restatement's PID rows (hp .. ld of the agents' slots: the device's MdPid rows under LaneChangePolicy); the
    oracle's own agent rows keep the other fields."""

    def __init__(self, host):
        import oracle_binding as ob
        from metadrive_ped_amd import abi
        self.host = host
        self.o = ob.OracleWorld(host)
        k = abi.MdConfig.from_buffer_copy(host.md_config)
        k.agent_idm = abi.AGENT_INPUT
        self.o.k = k
        self.pid = host.state["pid0"].copy()
        self.multi = bool(host.cfg["is_multi_agent"])

    @property
    def state(self):
        return self.o.state

    def reset(self):
        self.o.reset()
        self.pid = self.o.state["pid"].copy()

    def step(self, decoded):
        """decoded: [E, A, 2] float32, the env's decoded discrete actions -> the actions the oracle applied (before clipping)"""
        h, st = self.host, self.o.state
        a = h.world.arrays
        act = np.ascontiguousarray(np.asarray(decoded, np.float32).reshape(h.E, h.A, 2)).copy()
        lib().hx_lane_change_batch(_p(a["lanes"]), _p(a["lane_off"]), _p(a["roads"]), _p(a["road_off"]), _p(a["env_map"]),
                                   _p(st["shape"]), _p(st["dyn"]), _p(st["nav"]), _p(st["flags"]), _p(st["need_reset"]), _p(self.pid),
                                   _p(st["pid0"]), _p(act), h.E, h.cap, h.A, int(self.multi))
        ids = st["agent_id"].copy() if "agent_id" in st else None
        self.o.step(act)
        if ids is not None:     # a respawned agent gets a fresh policy: clean PIDs
            fresh = st["agent_id"] != ids
            for k in PID_ERRS:
                self.pid[k][fresh] = 0.0
        return act

    def agent_rows(self):
        """slot indices of the agents in the global [E * cap] arrays"""
        h = self.host
        return (np.arange(h.E)[:, None] * h.cap + np.arange(h.A)[None, :]).reshape(-1)


# the reference's known answer (tests/test_policy/test_lane_change_policy.py::test_lane_change)
CXO_CONFIG = dict(num_scenarios=1, traffic_density=0.0, start_seed=22, decision_repeat=5, map="CXO", agent_policy="LaneChangePolicy",
                  discrete_action=True, use_multi_discrete=True, action_check=True)
CXO_LEGS = (([2, 3], 59, 0), ([0, 3], 39, 2), ([1, 3], 69, 2))     # (action, steps, lane index after them)
