"""The host restatement of md_vector_obs (tests/vector_obs_host.c, the gcc build of include/md_vector_obs.h) on numpy arrays, and what
the vector-observation tests share: host-side output / history rows, the structs over a host scene or a downloaded device state,
hand-built one-lane worlds for the known answers.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
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
        self.outs, out_bytes, self.hists, hist_bytes = abi.vector_obs_blocks(self.cfg, A, cap)
        self.rows = np.zeros((E, out_bytes), np.uint8)
        self.hist = np.zeros((E, hist_bytes), np.uint8)
        ptrs = dict(out_stride=out_bytes, hist_stride=hist_bytes)
        for table, rows in ((self.outs, self.rows), (self.hists, self.hist)):
            for name, (off, shape, dt) in table.items():
                if int(np.prod(shape)):
                    ptrs[name] = rows.ctypes.data + off
        self.vo = abi.make_md_vector_obs(self.cfg, ptrs)

    @staticmethod
    def _block(rows, table, name):
        off, shape, dt = table[name]
        n = int(np.prod(shape)) * dt.itemsize
        return np.ascontiguousarray(rows[:, off:off + n]).view(dt).reshape((rows.shape[0], ) + tuple(shape))

    def out(self, name):
        """a copy of the block `name`, [E, A, ...]"""
        return self._block(self.rows, self.outs, name)

    def outputs(self):
        return {name: self.out(name) for name in abi.VECTOR_OBS_OUTPUTS}

    def history(self):
        return {name: self._block(self.hist, self.hists, name) for name in abi.VECTOR_OBS_HISTORY}

    def set_history(self, name, value):
        off, shape, dt = self.hists[name]
        n = int(np.prod(shape)) * dt.itemsize
        self.hist[:, off:off + n] = np.ascontiguousarray(value, dt).reshape(self.E, -1).view(np.uint8)

    def run(self, w, s, k):
        """one md_vector_obs call on host arrays"""
        assert lib().hx_vector_obs(C.byref(w), C.byref(s), C.byref(k), C.byref(self.vo)) == 0
        return self

    def push(self, s, k):
        assert lib().hx_vo_push(C.byref(s), C.byref(k), C.byref(self.vo)) == 0
        return self


def structs_of(host, state, env_map=None):
    """(MdWorld, MdState, MdConfig, keep-alive) over the host scene's tables and the numpy state `state` (the oracle's, or one
    downloaded from the device); env_map: the envs' maps when they are not the scene's own (a walking batch)"""
    from metadrive_ped_amd.engine import make_structs
    wa = dict(host.world.arrays, **host.world_scalars())
    if env_map is not None:
        wa["env_map"] = np.ascontiguousarray(env_map, np.int32)
    state = {k: np.ascontiguousarray(v) for k, v in state.items()}
    w, s, k = make_structs(wa, state, host.md_config, host.world.n_maps, host.E, hostlib.ptr)
    return w, s, k, (wa, state)


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
    w = abi.MdWorld()
    w.n_maps, w.n_envs, w.max_lanes, w.max_roads = 1, E, n_lanes, 1
    for k, v in world.items():
        setattr(w, k, hostlib.ptr(v))
    s = abi.MdState()
    for k, v in st.items():
        setattr(s, k, hostlib.ptr(v))
    k = abi.MdConfig()
    k.struct_size, k.n_envs, k.agents_per_env, k.cap, k.is_multi_agent = C.sizeof(abi.MdConfig), E, 1, cap, int(multi)
    return w, s, k, st, world


def put(st, slot, x, y, heading=0.0, kind=abi.KIND_VEHICLE, flags=abi.F_ALIVE, hl=2.25, hw=0.9, speed=0.0):
    import math
    sh = st["shape"][slot]
    sh["cx"], sh["cy"], sh["c"], sh["s"], sh["hl"], sh["hw"] = x, y, math.cos(heading), math.sin(heading), hl, hw
    sh["flags"], sh["aux"] = kind | flags, -1
    st["dyn"][slot]["heading"], st["dyn"][slot]["speed"] = heading, speed


def clear(st, slot):
    st["shape"][slot]["flags"] = 0
