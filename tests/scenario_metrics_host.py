"""The host restatement of md_scenario_metrics (tests/scenario_metrics_host.c, the gcc build of include/md_scenario_metrics.h) on numpy
arrays, and what the metrics tests share: host-side output and state rows as the engine lays them out, the structs over a host scene
with its recorded frames, and hand-built one-env worlds for the placed states.  TEST INFRASTRUCTURE."""
import ctypes as C
import math

import numpy as np

import hostlib
from hostlib import put     # noqa: F401  (the tests reach it through this module)
from metadrive_ped_amd import abi
from metadrive_ped_amd.config import check_scenario_metrics

_W, _S, _K, _M = C.POINTER(abi.MdWorld), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdScenarioMetrics)
OUTPUTS = abi.SCENARIO_METRICS_OUTPUTS
STEP, EPISODE = abi.SCENARIO_METRICS_STEP_COLUMNS.index, abi.SCENARIO_METRICS_EPISODE_COLUMNS.index
EGO_HL, EGO_HW = 2.25, 0.9
EGO_FLAGS = abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT
DT, SUBSTEPS = 0.02, 5


def _declare(lib):
    lib.hx_scenario_metrics.argtypes = [_W, _S, _K, _M]


def lib():
    return hostlib.build("scenario_metrics_host", _declare)


class HostScenarioMetrics:
    """Output rows and state rows as the engine lays them out (abi.scenario_metrics_blocks), in host memory, and the
    MdScenarioMetrics over them; `lights`: agent_light is read from self.agent_light [E] uint8 (else NULL: no lights configured)"""
    def __init__(self, sm_cfg, E, lights=False):
        self.cfg = check_scenario_metrics(dict(sm_cfg))
        self.E = E
        outs, out_bytes, state, state_bytes = abi.scenario_metrics_blocks(self.cfg)
        self._out, self._state = hostlib.HostRows(outs, out_bytes, E), hostlib.HostRows(state, state_bytes, E)
        self.rows, self.state = self._out.rows, self._state.rows
        self.agent_light = np.zeros(E, np.uint8)
        ptrs = dict(self._out.ptrs(), out_stride=out_bytes, state_stride=state_bytes, state=self.state.ctypes.data)
        if lights:
            ptrs.update(agent_light=self.agent_light.ctypes.data, light_stride=1)
        self.sm = abi.make_md_scenario_metrics(self.cfg, ptrs)

    def out(self, name):
        """a copy of the block `name`, [E, ...]: an output, or "episode" / "history" of the state rows"""
        return (self._out if name in self._out.table else self._state).out(name)

    def outputs(self):
        return {name: self.out(name) for name in OUTPUTS + ("episode", "history")}

    def history_i(self):
        return self.out("history").view(np.int32)

    def run(self, w, s, k):
        """one md_scenario_metrics call on host arrays"""
        assert lib().hx_scenario_metrics(C.byref(w), C.byref(s), C.byref(k), C.byref(self.sm)) == 0
        return self


def structs_of(host, state):
    """(MdWorld, MdState, MdConfig, keep-alive) over a scenario host scene and a downloaded state, with the scene's recorded frames and
    the walk in MdState as the engine sets them"""
    tr = host.tracks
    seen = dict(state, track_shape=np.ascontiguousarray(tr["shape"]), track_dyn=np.ascontiguousarray(tr["dyn"], np.float32))
    w, s, k, keep = hostlib.structs_of(host, seen)
    s.walk = abi.MdWalk(*host.walk_params)
    assert k.track_len == tr["shape"].shape[0]
    return w, s, k, keep


# -- hand-built worlds: ONE env, the observer in slot 0, T recorded frames of the SDC in slot 0 of the frame tables -----------------
def metrics_world(cap=8, T=16):
    st = dict(shape=np.zeros(cap, abi.SHAPE_DT), dyn=np.zeros(cap, abi.DYN_DT), nav=np.zeros(cap, abi.NAV_DT), flags=np.zeros(cap, np.uint32),
              step_info=np.zeros((1, 8), np.float32), track_shape=np.zeros((T, cap), abi.SHAPE_DT), track_dyn=np.zeros((T, cap, 2), np.float32))
    st["nav"]["lane"] = -1
    w, s, k = hostlib.hand_built_structs({}, st, cap=cap, traffic_mode=4, dt=DT, substeps=SUBSTEPS, scenario_length=T, track_len=T)
    return w, s, k, st


def put_ego(st, x, y, heading=0.0, speed=0.0, clock=1, flags=EGO_FLAGS, hl=EGO_HL, hw=EGO_HW):
    put(st, 0, x, y, heading, kind=0, flags=flags, hl=hl, hw=hw, speed=speed)
    st["nav"][0]["steps"] = clock


def put_frame(st, t, x, y, heading=0.0, flags=EGO_FLAGS):
    """the SDC's recorded frame t"""
    fr = st["track_shape"][t, 0]
    fr["cx"], fr["cy"], fr["c"], fr["s"], fr["hl"], fr["hw"], fr["flags"] = x, y, math.cos(heading), math.sin(heading), EGO_HL, EGO_HW, flags
    st["track_dyn"][t, 0] = (heading, 0.0)


def run_placed(movers, ego=(0.0, 0.0, 0.0, 10.0), cfg=None, clock=1, present=True, cap=8):
    """the host build on a one-env world with `movers` = (x, y, heading, speed[, hl, hw[, kind]]) in the slots 1 .. -> the outputs with
    the env axis dropped"""
    w, s, k, st = metrics_world(cap=cap)
    put_ego(st, ego[0], ego[1], ego[2], ego[3], clock=clock, flags=EGO_FLAGS if present else 0)
    for i, m in enumerate(movers):
        x, y, h, v = m[:4]
        hl, hw = (m[4], m[5]) if len(m) > 5 else (EGO_HL, EGO_HW)
        put(st, 1 + i, x, y, h, kind=m[6] if len(m) > 6 else abi.KIND_VEHICLE, hl=hl, hw=hw, speed=v)
    hm = HostScenarioMetrics(cfg or {}, 1).run(w, s, k)
    return {n: v[0] for n, v in hm.outputs().items()}


# -- the finite differences in float32 numpy, in the header's operation order ------------------------------------------------------
F = np.float32
PI_F, TWO_PI_F, INV_TWO_PI_F = F(3.14159265358979323846), F(6.28318530717958647692), F(0.15915494309189535)


def wrap_f32(x):
    """md_wrap_to_pi (include/md_math.h) on one float32, operation by operation"""
    x = F(x)
    a = F(x - F(TWO_PI_F * F(np.floor(F(x * INV_TWO_PI_F)))))
    if a < F(0):
        a = F(a + TWO_PI_F)
    if a >= TWO_PI_F:
        a = F(a - TWO_PI_F)
    if a > PI_F:
        a = F(a - TWO_PI_F)
    return a


def step_period():
    return F(F(DT) * F(SUBSTEPS))


def rates_f32(v, h, v0, h0, D):
    """columns 3 .. 5 from this step's and the previous step's speed and heading"""
    lon = F(F(F(v) - F(v0)) / D)
    yaw = F(wrap_f32(F(F(h) - F(h0))) / D)
    return lon, yaw, F(F(v) * yaw)


def jerks_f32(rates, rates0, D):
    """columns 6 .. 8 from this step's and the previous step's columns 3 .. 5"""
    lj = F(F(rates[0] - rates0[0]) / D)
    ya = F(F(rates[1] - rates0[1]) / D)
    latj = F(F(rates[2] - rates0[2]) / D)
    return lj, ya, F(np.sqrt(F(F(lj * lj) + F(latj * latj))))
