"""The host restatement of md_traffic_lights (tests/traffic_lights_host.c, the gcc build of include/md_traffic_lights.h) on numpy arrays,
and what the traffic-light tests share: host-side output rows with the light tables, the structs over a host scene, hand-built one-env
worlds for the placed states, a float64 numpy restatement of the flags (the box test is tests/contact_ref.py's) and a float32 one of
the selection.  TEST INFRASTRUCTURE."""
import ctypes as C
import math

import numpy as np

import contact_ref as cr
import hostlib
from hostlib import structs_of     # noqa: F401  (the tests reach it through this module)
from metadrive_ped_amd import abi
from metadrive_ped_amd.config import check_traffic_lights
from metadrive_ped_amd.scenario import traffic_light_tables

_W, _S, _K, _T = C.POINTER(abi.MdWorld), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdTrafficLights)
OUTPUTS = abi.TRAFFIC_LIGHTS_OUTPUTS
HL, HW = 0.125, 3.0          # the wall: AIR_WALL_LENGTH / 2 along the lane, VIS_LANE_WIDTH / 2 across it
EGO_HL, EGO_HW = 2.25, 0.9


def _declare(lib):
    lib.hx_traffic_lights.argtypes = [_W, _S, _K, _T]
    lib.hx_tl_constant.restype = C.c_float


def lib():
    return hostlib.build("traffic_lights_host", _declare)


class HostTrafficLights:
    """Output rows as the engine lays them out (abi.traffic_lights_blocks), in host memory, the light tables (`tables`:
    scenario.traffic_light_tables' dict, e.g. ScenarioHostScene.traffic_lights) and the MdTrafficLights over them"""
    def __init__(self, tl_cfg, E, tables):
        self.cfg = check_traffic_lights(dict(tl_cfg))
        self.E = E
        outs, out_bytes = abi.traffic_lights_blocks(self.cfg)
        self._out = hostlib.HostRows(outs, out_bytes, E)
        self.rows = self._out.rows
        self.tables = tables
        self._keep = {k: np.ascontiguousarray(tables[k]) for k in abi.TRAFFIC_LIGHTS_TABLES}
        ptrs = dict(self._out.ptrs(), out_stride=out_bytes, max_scene_lights=tables["max_scene_lights"])
        ptrs.update({k: v.ctypes.data for k, v in self._keep.items()})
        self.tl = abi.make_md_traffic_lights(self.cfg, ptrs)

    def out(self, name):
        """a copy of the block `name`, [E, ...]"""
        return self._out.out(name)

    def outputs(self):
        return self._out.outs()

    def run(self, w, s, k):
        """one md_traffic_lights call on host arrays"""
        assert lib().hx_traffic_lights(C.byref(w), C.byref(s), C.byref(k), C.byref(self.tl)) == 0
        return self


# -- hand-built worlds: ONE env, the observer in slot 0, the lights given as (x, y, heading, status codes) --------------------------
def light_tables(lights):
    """the tables of one scene whose lights are (x, y, heading of the wall's lane direction, [codes per frame])"""
    box = np.asarray([(x, y, math.cos(h), math.sin(h), HL, HW, 0.0, 0.0) for x, y, h, _ in lights], np.float32).reshape(-1, 8)
    return traffic_light_tables([(box, [np.asarray(c, np.uint8) for _, _, _, c in lights], list(range(len(lights))))])


def light_world(cap=8):
    st = dict(shape=np.zeros(cap, abi.SHAPE_DT), dyn=np.zeros(cap, abi.DYN_DT), nav=np.zeros(cap, abi.NAV_DT))
    st["nav"]["lane"] = -1
    w, s, k = hostlib.hand_built_structs({}, st, cap=cap, traffic_mode=4)
    return w, s, k, st


def put_ego(st, x, y, heading=0.0, flags=abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT, hl=EGO_HL, hw=EGO_HW, clock=1):
    sh = st["shape"][0]
    sh["cx"], sh["cy"], sh["c"], sh["s"], sh["hl"], sh["hw"] = x, y, math.cos(heading), math.sin(heading), hl, hw
    sh["flags"], sh["aux"] = flags, -1
    st["dyn"][0]["heading"] = heading
    st["nav"][0]["steps"] = clock


def run_world(lights, ego, clock=1, cfg=None, present=True):
    """the host build on a one-env world -> (outputs with the env axis dropped, tables)"""
    tables = light_tables(lights)
    w, s, k, st = light_world()
    put_ego(st, *ego, clock=clock, flags=(abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT) if present else 0)
    hv = HostTrafficLights(cfg or {}, 1, tables).run(w, s, k)
    return {n: v[0] for n, v in hv.outputs().items()}, tables, st


# -- the rule in numpy: the flags in float64 over contact_ref's box test, the selection in float32 ---------------------------------
def frame_code(tables, at, f):
    off, n = int(tables["tl_info"][at, 0]), int(tables["tl_info"][at, 1])
    return int(tables["tl_status"][off + min(max(f, 0), n - 1)])


def ref_agent_light(me, tables, scene, t):
    """-> (bits, decided): `me` one MdShape record [1]; every overlapped wall's acting status; decided where the chassis grown and
    shrunk by contact_ref.EPS agree on every wall that could raise a bit"""
    a, b = int(tables["tl_off"][scene]), int(tables["tl_off"][scene + 1])
    present = bool(me["flags"][0] & abi.F_ALIVE) and (int(me["flags"][0]) & abi.KIND_MASK) != abi.KIND_NONE
    if t < 1 or not present or b == a:
        return 0, True
    box = tables["tl_box"][a:b]
    walls = cr.make_shapes(box[:, 0], box[:, 1], np.arctan2(box[:, 3].astype(np.float64), box[:, 2].astype(np.float64)), box[:, 4], box[:, 5])
    hit, decided = cr.obb_obb(np.repeat(me, b - a), walls)
    bits, ok = 0, True
    for q in range(b - a):
        code = frame_code(tables, a + q, t - 1)
        if code == 0:
            continue
        ok = ok and bool(decided[q])
        if hit[q]:
            bits |= 1 << (code - 1)
    return bits, ok


def ref_lights(tables, scene, cx, cy, c, s, radius, L, t):
    """-> (lights [L, 6], lights_mask [L], lights_index [L]) for a valid observer at (cx, cy) with heading vector (c, s), in float32"""
    f = np.float32
    a, b = int(tables["tl_off"][scene]), int(tables["tl_off"][scene + 1])
    out, mask, index = np.zeros((L, 6), f), np.zeros(L, np.uint8), np.full(L, -1, np.int32)
    if b == a:
        return out, mask, index
    box, info = tables["tl_box"][a:b].astype(f), tables["tl_info"][a:b]
    dx, dy = box[:, 0] - f(cx), box[:, 1] - f(cy)
    d2 = dx * dx + dy * dy
    cand = np.nonzero(d2 <= f(radius) * f(radius))[0]
    order = cand[np.lexsort((info[cand, 2], d2[cand]))][:L]
    for r, q in enumerate(order):
        out[r] = (dx[q] * f(c) + dy[q] * f(s), dy[q] * f(c) - dx[q] * f(s), box[q, 2] * f(c) + box[q, 3] * f(s),
                  box[q, 3] * f(c) - box[q, 2] * f(s), frame_code(tables, a + q, t), d2[q])
        mask[r], index[r] = 1, info[q, 2]
    return out, mask, index
