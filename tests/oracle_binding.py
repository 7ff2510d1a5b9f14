"""ctypes binding of the CPU oracle (oracle/_build/libmdoracle.so).  TEST INFRASTRUCTURE: imported by
tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg only -- never by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

from metadrive_ped_amd import abi
from metadrive_ped_amd.engine import make_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "_build", "libmdoracle.so")
_LIBS = {}


def build():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR])


def load(path=None):
    """path: another build of the same source (bench.py's -O3 -march=native one); default = the -O2 checker."""
    path = path or ORACLE_SO
    if path in _LIBS:
        return _LIBS[path]
    if path == ORACLE_SO:
        build()     # make: a no-op when up to date, so a stale oracle never checks a newer header
    lib = C.CDLL(path)
    W, S, K = C.POINTER(abi.MdWorld), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig)
    for name in ("ref_integrate", "ref_localize", "ref_contacts", "ref_observe", "ref_idm", "ref_traffic_after_step",
                 "ref_lifecycle", "ref_step"):
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [W, S, K]
    lib.ref_step_mt.restype = C.c_int
    lib.ref_step_mt.argtypes = [W, S, K, C.c_int]
    lib.ref_lidar.restype = C.c_int
    lib.ref_lidar.argtypes = [W, S, K, C.c_void_p, C.c_int, C.c_int]
    lib.ref_line_detector.restype = C.c_int
    lib.ref_line_detector.argtypes = [W, S, K, C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_int, C.c_int]
    lib.ref_abi.restype = C.c_int
    lib.ref_abi.argtypes = [C.POINTER(C.c_int32), C.c_int]
    lib.ref_scenario_after_step.restype = C.c_int
    lib.ref_scenario_after_step.argtypes = [W, S, K, C.c_int, C.c_int]
    lib.ref_build_route.restype = C.c_int
    lib.ref_build_route.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.ref_others_block.restype = C.c_int
    lib.ref_others_block.argtypes = [W, S, K, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    f = C.c_float
    lib.ref_lane_local.argtypes = [C.c_void_p, f, f, C.c_void_p]
    lib.ref_lane_heading_at.restype = f
    lib.ref_lane_heading_at.argtypes = [C.c_void_p, f]
    lib.ref_heading_diff.restype = f
    lib.ref_heading_diff.argtypes = [C.c_void_p, f, f, f, f]
    lib.ref_navi.argtypes = [C.c_void_p, f, f, f, f, f, f, f, C.c_void_p]
    lib.ref_idm_acc.restype = f
    lib.ref_idm_acc.argtypes = [f, f, C.c_int, f, f]
    lib.ref_pid.restype = f
    lib.ref_pid.argtypes = [C.c_void_p, f, f, f, f]
    lib.ref_wrap_to_pi.restype = f
    lib.ref_wrap_to_pi.argtypes = [f]
    lib.ref_sincos.argtypes = [f, C.c_void_p]
    lib.ref_atan2.restype = f
    lib.ref_atan2.argtypes = [f, f]
    lib.ref_acos.restype = f
    lib.ref_acos.argtypes = [f]
    lib.ref_sanitize.restype = f
    lib.ref_sanitize.argtypes = [f]
    lib.ref_ray_shape.restype = f
    lib.ref_ray_shape.argtypes = [f, f, f, f, C.c_void_p]
    lib.ref_obb_obb.restype = C.c_int
    lib.ref_obb_obb.argtypes = [C.c_void_p, C.c_void_p]
    lib.ref_obb_circle.restype = C.c_int
    lib.ref_obb_circle.argtypes = [C.c_void_p, f, f, f]
    lib.ref_obb_quad.restype = C.c_int
    lib.ref_obb_quad.argtypes = [C.c_void_p, C.c_void_p]
    lib.ref_bicycle.argtypes = [C.c_void_p, f, f, C.c_void_p, f, C.c_int]
    lib.ref_idm_gap.restype = f
    lib.ref_idm_gap.argtypes = [f, f]
    lib.ref_idm_steer.restype = f
    lib.ref_idm_steer.argtypes = [C.c_void_p, f, f, f, C.c_void_p]
    lib.ref_front_back.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, f, f, C.c_void_p, C.c_void_p]
    lib.ref_idm_vehicle.restype = None
    lib.ref_idm_vehicle.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.ref_scenario_observe.restype = C.c_int
    lib.ref_scenario_observe.argtypes = [W, S, K]
    lib.ref_tidm_vehicle.restype = C.c_int
    lib.ref_tidm_vehicle.argtypes = [W, S, K, C.c_int, C.c_int, C.c_int]
    lib.ref_poly_local.argtypes = [C.c_void_p, C.c_int, f, f, C.c_void_p]
    lib.ref_poly_position.argtypes = [C.c_void_p, C.c_int, f, f, C.c_void_p]
    lib.ref_traj_navi.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, f, f, f, f, C.c_void_p]
    lib.ref_point_in_polygon.restype = C.c_int
    lib.ref_point_in_polygon.argtypes = [C.c_void_p, C.c_int, f, f]
    lib.ref_probe_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    abi.check_abi(lib.ref_abi, path)
    _LIBS[path] = lib
    return lib


def _ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


class OracleWorld:
    """The oracle running on a HostScene's tables with its own copy of the state."""
    def __init__(self, host, state=None, lib=None):
        self.lib = lib or load()
        self.host = host
        self.state = state if state is not None else host.clone_state()
        wa = dict(host.world.arrays, **host.world_scalars())
        self.w, self.s, self.k = make_structs(wa, self.state, host.md_config, host.world.n_maps, host.E, _ptr)

    def call(self, name, *extra):
        rc = getattr(self.lib, name)(C.byref(self.w), C.byref(self.s), C.byref(self.k), *extra)
        assert rc == 0, (name, rc)

    def step(self, actions=None, threads=1):
        self._held = None
        if actions is not None and not self.k.agent_idm:
            # like BatchedEngine.step: hand the agents' actions over through MdState.agent_action
            self._held = np.ascontiguousarray(np.asarray(actions, np.float32).reshape(self.host.E, self.host.A, 2))
            self.s.agent_action = self._held.ctypes.data
        try:
            if threads > 1:
                self.call("ref_step_mt", threads)
            else:
                self.call("ref_step")
        finally:
            self.s.agent_action = None
        self._detectors()

    def _detectors(self):
        from metadrive_ped_amd.engine import BatchedEngine
        h = self.host
        vc = h.cfg["vehicle_config"]
        if h.n_side:
            self.call("ref_line_detector", C.c_void_p(h.side_beams.ctypes.data), h.n_side, C.c_float(vc["side_detector"]["distance"]),
                      C.c_uint32(BatchedEngine.SIDE_MASK), C.c_void_p(self.state["obs"].ctypes.data), h.obs_dim, h.obs_base)
        if h.n_ll:
            self.call("ref_line_detector", C.c_void_p(h.ll_beams.ctypes.data), h.n_ll, C.c_float(vc["lane_line_detector"]["distance"]),
                      C.c_uint32(BatchedEngine.LANE_LINE_MASK), C.c_void_p(self.state["obs"].ctypes.data), h.obs_dim,
                      h.obs_base + (h.n_side or 2) + 6)

    def set_tracks(self, shape, dyn):
        """traffic_mode 'replay': frames [T, E*cap] of MdShape records and [T, E*cap, 2] (heading, speed)."""
        self._track_shape = np.ascontiguousarray(shape)
        self._track_dyn = np.ascontiguousarray(dyn, np.float32)
        self.s.track_shape = self._track_shape.ctypes.data
        self.s.track_dyn = self._track_dyn.ctypes.data
        self.k.track_len = int(self._track_shape.shape[0])

    def reset(self):
        self.state["need_reset"][:] = 1
        self.call("ref_step")
        self._detectors()

    def lidar(self):
        out = np.zeros((self.host.E * self.host.A, self.host.n_beams), np.float32)
        self.call("ref_lidar", C.c_void_p(out.ctypes.data), self.host.n_beams, 0)
        return out

    @property
    def obs(self):
        return self.state["obs"]


def record_episode(o, actions):
    """Drive OracleWorld `o` (already reset) through `actions` and return the frames in BatchedEngine.stop_recording's
    layout: frame 0 = the reset state, frame k = the state after step k."""
    T, n = len(actions), o.host.E * o.host.cap
    shape = np.zeros((T + 1, n), dtype=abi.SHAPE_DT)
    dyn = np.zeros((T + 1, n, 2), np.float32)
    for k in range(T + 1):
        if k:
            o.step(actions[k - 1])
        shape[k] = o.state["shape"]
        dyn[k, :, 0] = o.state["dyn"]["heading"]
        dyn[k, :, 1] = o.state["dyn"]["speed"]
    return dict(shape=shape, dyn=dyn, seeds=list(o.host.seeds), cap=o.host.cap)


def lidar_raw(shape, beam_cs, E, cap, n_beams, lidar_range, agents_per_env=1):
    """ref_lidar on a bare shape table (the agents of an env in its first slots; rows [E * agents_per_env, n_beams]): the lidar
    micro-bench's checker."""
    lib = load()
    A = agents_per_env
    shape = np.ascontiguousarray(shape)
    beam_cs = np.ascontiguousarray(beam_cs, np.float32)
    w = abi.MdWorld()
    w.n_maps, w.n_envs, w.max_lanes, w.max_roads = 1, E, 1, 1
    w.beam_cs = beam_cs.ctypes.data
    s = abi.MdState()
    s.shape = shape.ctypes.data
    k = abi.MdConfig()
    k.struct_size = C.sizeof(abi.MdConfig)
    k.n_envs, k.agents_per_env, k.cap, k.n_beams, k.obs_dim = E, A, cap, n_beams, n_beams
    k.lidar_range = lidar_range
    out = np.zeros((E * A, n_beams), np.float32)
    rc = lib.ref_lidar(C.byref(w), C.byref(s), C.byref(k), C.c_void_p(out.ctypes.data), n_beams, 0)
    assert rc == 0
    return out


def bare_detector_structs(E, cap, A, ptr):
    """MdWorld / MdState / MdConfig for the line detectors on bare tables: ptr(name) -> the address of quads, quad_kind, quad_off,
    env_map, shape and (0 = NULL) quad_ball"""
    w = abi.MdWorld()
    w.n_maps, w.n_envs, w.max_lanes, w.max_roads = E, E, 1, 1
    w.env_map, w.quad_off, w.quads, w.quad_kind = ptr("env_map"), ptr("quad_off"), ptr("quads"), ptr("quad_kind")
    w.quad_ball = ptr("quad_ball") or None
    s = abi.MdState()
    s.shape = ptr("shape")
    k = abi.MdConfig()
    k.struct_size = C.sizeof(abi.MdConfig)
    k.n_envs, k.agents_per_env, k.cap = E, A, cap
    return w, s, k


def line_detector_raw(world, beam_cs, rng, mask):
    """ref_line_detector on bare tables (a dict of quads, quad_kind, quad_off, env_map, shape [E, cap]; the agents are the slots
    0 .. cap-1) -> [E * cap, n]"""
    lib = load()
    held = {k: np.ascontiguousarray(v) for k, v in world.items()}
    beam_cs = np.ascontiguousarray(beam_cs, np.float32)
    E, cap = held["shape"].shape
    w, s, k = bare_detector_structs(E, cap, cap, lambda name: held[name].ctypes.data if name in held else 0)
    out = np.zeros((E * cap, len(beam_cs)), np.float32)
    rc = lib.ref_line_detector(C.byref(w), C.byref(s), C.byref(k), C.c_void_p(beam_cs.ctypes.data), len(beam_cs), C.c_float(rng),
                               C.c_uint32(mask), C.c_void_p(out.ctypes.data), len(beam_cs), 0)
    assert rc == 0
    return out


def build_route(points, seg_cap=None, vert_cap=None):
    """md_build_route (include/md_scenario.h) on a point list -> (pieces SEG_DT, outline [n, 2], aux [8], rc)"""
    import numpy as np
    from metadrive_ped_amd import abi
    pts = np.ascontiguousarray(np.asarray(points, np.float32)[:, :2])
    seg_cap = seg_cap or max(1, len(pts))
    if vert_cap is None:
        d = np.diff(pts.astype(np.float64), axis=0)
        vert_cap = 2 * (int(np.ceil(np.sqrt((d ** 2).sum(1)).sum())) + 3) + 4
    segs = np.zeros(seg_cap, dtype=abi.SEG_DT)
    verts = np.zeros((vert_cap, 2), np.float32)
    aux = np.zeros(8, np.float32)
    counts = np.zeros(2, np.int32)
    rc = load().ref_build_route(pts.ctypes.data, len(pts), segs.ctypes.data, seg_cap, verts.ctypes.data, vert_cap, aux.ctypes.data,
                                counts.ctypes.data)
    return segs[:counts[0]], verts[:counts[1]], aux, rc
