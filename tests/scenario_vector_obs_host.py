"""The host restatement of md_scenario_vector_obs (tests/scenario_vector_obs_host.c, the gcc build of
include/md_scenario_vector_obs.h) on numpy arrays, and what the scenario vector-observation tests share: host-side output / history
rows with the piece tables, the structs over a host scene, hand-built one-trajectory worlds for the known answers, and a numpy float32
restatement of the map selection.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
from hostlib import put, structs_of     # noqa: F401  (the tests reach them through this module)
from metadrive_ped_amd import abi
from metadrive_ped_amd.config import check_scenario_vector_obs
from metadrive_ped_amd.scenario import map_piece_tables

_W, _S, _K, _V = C.POINTER(abi.MdWorld), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdScenarioVectorObs)
# the smallest shapes that can still go wrong
SMALL = dict(num_agents=3, history=3, route_points=5, num_pieces=3, piece_points=3)
CEILINGS = dict(num_agents=16, history=8, route_points=32, num_pieces=64, piece_points=16)
OUTPUTS, HISTORY = abi.SCENARIO_VECTOR_OBS_OUTPUTS, abi.VECTOR_OBS_HISTORY


def _declare(lib):
    lib.hx_scenario_vector_obs.argtypes = [_W, _S, _K, _V]


def lib():
    return hostlib.build("scenario_vector_obs_host", _declare)


class HostScenarioVectorObs:
    """Output rows and history rows as the engine lays them out (abi.scenario_vector_obs_blocks), in host memory, the piece tables
    (`pieces`: scenario.map_piece_tables' dict, e.g. ScenarioHostScene.map_pieces) and the MdScenarioVectorObs over them"""
    def __init__(self, vo_cfg, E, cap, pieces=None):
        self.cfg = check_scenario_vector_obs(dict(vo_cfg))
        self.E = E
        outs, out_bytes, hists, hist_bytes = abi.scenario_vector_obs_blocks(self.cfg, cap)
        self._out, self._hist = hostlib.HostRows(outs, out_bytes, E), hostlib.HostRows(hists, hist_bytes, E)
        self.rows, self.hist = self._out.rows, self._hist.rows
        ptrs = dict(self._out.ptrs(), out_stride=out_bytes, hist_stride=hist_bytes, max_pieces=0, **self._hist.ptrs())
        self.pieces = pieces
        if pieces is not None and self.cfg["num_pieces"] > 0:
            self._keep = {k: np.ascontiguousarray(pieces[k]) for k in abi.SCENARIO_VECTOR_OBS_TABLES}
            ptrs.update({k: v.ctypes.data for k, v in self._keep.items()}, max_pieces=pieces["max_pieces"])
        self.sv = abi.make_md_scenario_vector_obs(self.cfg, ptrs)

    def out(self, name):
        """a copy of the block `name`, [E, ...]"""
        return self._out.out(name)

    def outputs(self):
        return self._out.outs()

    def history(self):
        return self._hist.outs()

    def run(self, w, s, k):
        """one md_scenario_vector_obs call on host arrays"""
        assert lib().hx_scenario_vector_obs(C.byref(w), C.byref(s), C.byref(k), C.byref(self.sv)) == 0
        return self


# -- hand-built worlds: ONE env whose reference trajectory is the polyline through `points`, the observer in slot 0 ------------------
def trajectory_world(points, cap=8):
    from metadrive_ped_amd.scenario import PolyLine
    segs = PolyLine(np.asarray(points, np.float64)).records()
    world = dict(poly_off=np.asarray([0, len(segs)] + [len(segs)] * (cap - 1), np.int32), segs=segs)
    st = dict(shape=np.zeros(cap, abi.SHAPE_DT), dyn=np.zeros(cap, abi.DYN_DT), nav=np.zeros(cap, abi.NAV_DT))
    st["nav"]["lane"] = -1
    w, s, k = hostlib.hand_built_structs(world, st, cap=cap, traffic_mode=4)
    return w, s, k, st, world


def pieces_of(features, spacing, S):
    """the tables of one scene with these map_features"""
    from metadrive_ped_amd.scenario import scene_map_pieces
    return map_piece_tables([scene_map_pieces(features, spacing, S)], S)


# -- the map selection in numpy float32, one env: what the header's plain loops state ------------------------------------------------
def select_pieces(pieces, scene, cx, cy, c, s, map_radius, P, S):
    """-> (map [P, S, 2], map_mask [P, S], map_meta [P, 4]) for an observer at (cx, cy) with heading vector (c, s)"""
    f = np.float32
    a, b = int(pieces["map_off"][scene]), int(pieces["map_off"][scene + 1])
    xy, info = pieces["map_xy"][a:b].astype(f), pieces["map_info"][a:b]
    out, mask, meta = np.zeros((P, S, 2), f), np.zeros((P, S), np.uint8), np.zeros((P, 4), f)
    if b == a:
        return out, mask, meta
    dx, dy = xy[:, :, 0] - f(cx), xy[:, :, 1] - f(cy)
    d2 = dx * dx + dy * dy                                        # float32 products and sum, like the header
    real = np.arange(S)[None, :] < info[:, 2][:, None]
    d2 = np.where(real, d2, f(np.inf)).min(1)
    cand = np.nonzero(d2 <= f(map_radius) * f(map_radius))[0]
    order = cand[np.lexsort((cand, d2[cand]))][:P]
    for p, q in enumerate(order):
        n = int(info[q, 2])
        rx, ry = xy[q, :n, 0] - f(cx), xy[q, :n, 1] - f(cy)
        out[p, :n, 0] = rx * f(c) + ry * f(s)
        out[p, :n, 1] = ry * f(c) - rx * f(s)
        mask[p, :n] = 1
        meta[p] = (info[q, 0], info[q, 1], n, d2[q])
    return out, mask, meta
