"""The host restatement of md_vector_obs (tests/vector_obs_host.c, the gcc build of include/md_vector_obs.h) on numpy arrays, and what
the vector-observation tests share: host-side output / history rows, the structs over a host scene or a downloaded device state,
hand-built one-lane worlds for the known answers.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
from hostlib import clear, put, structs_of     # noqa: F401  (the tests reach them through this module)
from metadrive_ped_amd import abi
from metadrive_ped_amd.config import check_vector_obs

_W, _S, _K, _V = C.POINTER(abi.MdWorld), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdVectorObs)
SMALL = dict(num_agents=3, history=3, route_points=5, num_lanes=3, lane_points=3)     # the smallest shapes that can still go wrong


def _declare(lib):
    lib.hx_vector_obs.argtypes = [_W, _S, _K, _V]
    lib.hx_vo_push.argtypes = [_S, _K, _V]
    lib.hx_vo_lane_local.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    lib.hx_vo_lane_local.restype = None


def lib():
    return hostlib.build("vector_obs_host", _declare)


class HostVectorObs:
    """Output rows and history rows as the engine lays them out (abi.vector_obs_blocks), in host memory, and the MdVectorObs over
    them"""
    def __init__(self, vo_cfg, E, A, cap):
        self.cfg = check_vector_obs(dict(vo_cfg))
        self.E = E
        outs, out_bytes, hists, hist_bytes = abi.vector_obs_blocks(self.cfg, A, cap)
        self._out, self._hist = hostlib.HostRows(outs, out_bytes, E), hostlib.HostRows(hists, hist_bytes, E)
        self.rows, self.hist = self._out.rows, self._hist.rows
        self.vo = abi.make_md_vector_obs(self.cfg, dict(self._out.ptrs(), out_stride=out_bytes, hist_stride=hist_bytes, **self._hist.ptrs()))

    def out(self, name):
        """a copy of the block `name`, [E, A, ...]"""
        return self._out.out(name)

    def outputs(self):
        return self._out.outs()

    def history(self):
        return self._hist.outs()

    def set_history(self, name, value):
        self._hist.set(name, value)

    def run(self, w, s, k):
        """one md_vector_obs call on host arrays"""
        assert lib().hx_vector_obs(C.byref(w), C.byref(s), C.byref(k), C.byref(self.vo)) == 0
        return self

    def push(self, s, k):
        assert lib().hx_vo_push(C.byref(s), C.byref(k), C.byref(self.vo)) == 0
        return self


def lane_local(lane_record, x, y):
    """md_lane_local of the host build: (longitudinal, lateral) of (x, y) on the LANE_DT record"""
    rec = np.ascontiguousarray(np.asarray(lane_record, abi.LANE_DT).reshape(1))
    out = np.zeros(2, np.float32)
    lib().hx_vo_lane_local(rec.ctypes.data, float(x), float(y), out.ctypes.data)
    return float(out[0]), float(out[1])


# -- hand-built worlds: one straight road of `n_lanes` lanes along +x from the origin, the observer in slot 0 --------------------
def straight_world(E=1, cap=8, n_lanes=1, length=200.0, width=3.5, multi=False):
    lanes = np.zeros(n_lanes, abi.LANE_DT)
    for i in range(n_lanes):
        L = lanes[i]
        L["type"], L["road"], L["idx"], L["n_in_road"] = 0, 0, i, n_lanes
        L["ax"], L["ay"], L["bx"], L["by"] = 0.0, -width * i, 1.0, 0.0
        L["length"], L["width"], L["heading"] = length, width, 0.0
        L["sx"], L["sy"], L["ex"], L["ey"] = 0.0, -width * i, length, -width * i
    roads = np.zeros(1, abi.ROAD_DT)
    roads[0]["first_lane"], roads[0]["n_lanes"], roads[0]["start_node"], roads[0]["end_node"] = 0, n_lanes, 0, 1
    world = dict(env_map=np.zeros(E, np.int32), lane_off=np.asarray([0, n_lanes], np.int32), lanes=lanes,
                 road_off=np.asarray([0, 1], np.int32), roads=roads)
    n = E * cap
    st = dict(shape=np.zeros(n, abi.SHAPE_DT), dyn=np.zeros(n, abi.DYN_DT), nav=np.zeros(n, abi.NAV_DT),
              route_roads=np.full((n, abi.MD_ROUTE_LEN), -1, np.int32), final_lane=np.zeros(n, np.int32), env_steps=np.zeros(E, np.int32))
    st["nav"]["lane"] = -1
    for e in range(E):
        put(st, e * cap, 0.0, 0.0, 0.0, flags=abi.F_ALIVE | abi.F_AGENT)
        nav = st["nav"][e * cap]
        nav["lane"], nav["ck0"], nav["ck1"], nav["route_len"], nav["road0"], nav["road1"] = 0, 0, 0, 2, 0, 0
        st["route_roads"][e * cap, 0] = 0
    w, s, k = hostlib.hand_built_structs(dict(world, max_lanes=n_lanes, max_roads=1), st, n_envs=E, cap=cap, is_multi_agent=int(multi))
    return w, s, k, st, world
