"""The host restatement of md_ped (tests/ped_host.c, the gcc build of include/md_ped.h) applied to numpy state arrays, and what the
pedestrian tests share: hand-built states for the known answers, the rule + oracle rollout, the coverage counters.
TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
from metadrive_ped_amd import abi

_S, _K, _P = C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdPed)


def _declare(lib):
    lib.hx_ped.argtypes = [_S, _K, _P]
    lib.hx_ped_vehicle.argtypes = [_S, _P, C.c_int, C.c_int]


def lib():
    return hostlib.build("ped_host", _declare)


DEFAULTS = dict(speed=1.2, wait_min_steps=10, clear_dist=1.0, margin=1.0, time_margin=1.0, yield_ahead=3.0, yield_time=1.5)


def state_struct(state):
    """abi.MdState over the numpy arrays `state` (the fields the rule touches)"""
    s = abi.MdState()
    for k in ("shape", "dyn", "nav", "pid", "idm_rand", "need_reset"):
        setattr(s, k, hostlib.ptr(state[k]))
    return s


def config_struct(E, cap, dt=0.02, substeps=5):
    k = abi.MdConfig()
    k.struct_size, k.n_envs, k.agents_per_env, k.cap, k.dt, k.substeps = C.sizeof(abi.MdConfig), E, 1, cap, dt, substeps
    return k


def apply(state, k, ped):
    """One md_ped launch on host arrays"""
    assert lib().hx_ped(C.byref(state_struct(state)), C.byref(k), C.byref(ped)) == 0


def walk(state, k):
    """What md_step does with walking participants (md_walk_mover, include/md_entity.h), for the hand-built states that run
    without the oracle: position += velocity * step_dt in float32"""
    sh, d = state["shape"], state["dyn"]
    step_dt = np.float32(k.dt) * np.float32(k.substeps)
    for j in range(len(sh)):
        f = int(sh["flags"][j])
        if (f & abi.F_ALIVE) and not (f & abi.F_STATIC) and (f & abi.KIND_MASK) in (abi.KIND_PEDESTRIAN, abi.KIND_CYCLIST):
            d["last_x"][j], d["last_y"][j] = sh["cx"][j], sh["cy"][j]
            sh["cx"][j] = np.float32(sh["cx"][j] + np.float32(d["steering"][j] * step_dt))
            sh["cy"][j] = np.float32(sh["cy"][j] + np.float32(d["throttle"][j] * step_dt))


def blank_state(cap, E=1):
    st = dict(shape=np.zeros(E * cap, abi.SHAPE_DT), dyn=np.zeros(E * cap, abi.DYN_DT), nav=np.zeros(E * cap, abi.NAV_DT),
              pid=np.zeros(E * cap, abi.PID_DT), idm_rand=np.zeros((E * cap, abi.MD_IDM_RAND), np.int32), need_reset=np.zeros(E, np.int32))
    st["shape"]["aux"] = -1
    st["nav"]["lane"] = -1
    return st


def put_pedestrian(st, slot, A, B, phase=abi.PED_WAIT_A, countdown=0, speed=1.2, draws=(0, ) * 8, at=None):
    """A policy-driven pedestrian in `slot`, standing at A (phases 1, 2) or B, or at `at`"""
    import math
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    h = math.atan2(float(B[1]) - float(A[1]), float(B[0]) - float(A[0]))
    hb = math.atan2(float(A[1]) - float(B[1]), float(A[0]) - float(B[0]))
    pos = (A if phase <= abi.PED_CROSS_AB else B) if at is None else np.asarray(at, np.float32)
    sh = st["shape"][slot]
    sh["cx"], sh["cy"], sh["c"], sh["s"], sh["hl"], sh["hw"] = pos[0], pos[1], math.cos(h), math.sin(h), 0.35, 0.35
    sh["flags"], sh["aux"] = abi.KIND_PEDESTRIAN | abi.F_ALIVE, -1
    st["dyn"][slot]["heading"] = h
    p = st["pid"][slot]
    p["hp"], p["hi"], p["hd"], p["lp"], p["li"], p["ld"], p["target_speed"] = A[0], A[1], B[0], B[1], speed, h, hb
    st["nav"][slot]["toll_state"], st["nav"][slot]["timer"], st["nav"][slot]["rand_cursor"] = phase, countdown, 0
    st["idm_rand"][slot] = draws


def put_vehicle(st, slot, x, y, heading, speed, hl=2.25, hw=0.9, flags=abi.F_ALIVE):
    import math
    sh = st["shape"][slot]
    sh["cx"], sh["cy"], sh["c"], sh["s"], sh["hl"], sh["hw"] = x, y, math.cos(heading), math.sin(heading), hl, hw
    sh["flags"] = abi.KIND_VEHICLE | flags
    st["dyn"][slot]["heading"], st["dyn"][slot]["speed"] = heading, speed


def driven_slots(state, E, cap):
    """[E, cap] bool: the policy-driven pedestrians"""
    f = state["shape"]["flags"].reshape(E, cap)
    return ((f & abi.KIND_MASK) == abi.KIND_PEDESTRIAN) & ((f & abi.F_ALIVE) != 0) & ((f & abi.F_STATIC) == 0) & \
        (state["nav"]["toll_state"].reshape(E, cap) != 0)


class Coverage:
    """What a rollout showed of the rule, read off the state before and after each md_ped: the phases reached, kerb holds (a
    waiting pedestrian whose countdown is 0 stays), mid-crossing stops (a crossing pedestrian short of its end point with velocity
    0), wait draws."""
    def __init__(self):
        self.phases, self.kerb_holds, self.mid_stops, self.arrivals = set(), 0, 0, 0

    def note(self, before, after, E, cap):
        m = driven_slots(before, E, cap) & (before["need_reset"] == 0)[:, None]
        p0, p1 = before["nav"]["toll_state"].reshape(E, cap)[m], after["nav"]["toll_state"].reshape(E, cap)[m]
        t0 = before["nav"]["timer"].reshape(E, cap)[m]
        v1 = after["dyn"]["speed"].reshape(E, cap)[m]
        self.phases |= set(int(p) for p in p1)
        waiting0 = (p0 == abi.PED_WAIT_A) | (p0 == abi.PED_WAIT_B)
        crossing1 = (p1 == abi.PED_CROSS_AB) | (p1 == abi.PED_CROSS_BA)
        self.kerb_holds += int((waiting0 & (t0 <= 1) & (p1 == p0) & (after["nav"]["timer"].reshape(E, cap)[m] == 0)).sum())
        self.mid_stops += int((crossing1 & ~waiting0 & (v1 == 0.0)).sum())
        self.arrivals += int((~waiting0 & ~crossing1).sum())


def rollout(host, steps, actions_of, ped=None, cover=None, each=None):
    """The rule + the oracle over `steps` steps from the host scene's reset: md_ped on orc.state before every orc.step.
    each(t, orc) runs after every step."""
    import oracle_binding as ob
    orc = ob.OracleWorld(host)
    ped = ped or abi.make_md_ped(host.cfg["pedestrian_config"])
    for t in range(-1, steps):
        before = {k: orc.state[k].copy() for k in ("shape", "nav", "need_reset")} if cover is not None else None
        apply(orc.state, orc.k, ped)
        if cover is not None:
            cover.note(before, orc.state, host.E, host.cap)
        if t < 0:
            orc.reset()        # need_reset is 1 everywhere: md_ped skipped every env, as on the device
        else:
            orc.step(actions_of(t))
            if each is not None:
                each(t, orc)
    return orc
