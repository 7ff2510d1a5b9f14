"""The host restatement of md_contact_response (tests/contact_response_host.c, the gcc build of include/md_contact_response.h)
applied to numpy state arrays, and what the contact response tests share: placed-state builders, the pair evaluator, the rule +
oracle wrapper and the coverage counters.  TEST INFRASTRUCTURE."""
import ctypes as C
import math

import numpy as np

import hostlib
from metadrive_ped_amd import abi
from ped_host import blank_state, config_struct      # the same hand-built state arrays; MdConfig with the sizes  # noqa: F401

_S, _K, _CR = C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdContactResponse)
DEFAULTS = dict(skin=0.01, max_push=0.5)
VEH = abi.KIND_VEHICLE | abi.F_ALIVE


def _declare(lib):
    lib.hx_contact_response.argtypes = [_S, _K, _CR]
    lib.hx_cr_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hx_cr_contacts.restype = None


def lib():
    return hostlib.build("contact_response_host", _declare)


def params(**kw):
    return abi.make_md_contact_response(dict(DEFAULTS, **kw))


def state_struct(state):
    """abi.MdState over the numpy arrays `state` (the fields the rule touches)"""
    s = abi.MdState()
    for k in ("shape", "dyn", "need_reset"):
        setattr(s, k, hostlib.ptr(state[k]))
    return s


def apply(state, k, cr):
    """One md_contact_response launch on host arrays"""
    assert lib().hx_contact_response(C.byref(state_struct(state)), C.byref(k), C.byref(cr)) == 0


def contacts(I, si, J, sj):
    """Responder records I (MdShape, boxes) in slots si against obstacle records J in slots sj -> (hit [n] bool, depth, nx, ny,
    near [n] bool: the cull lets the pair through, ref [n] bool: md_obb_obb / md_obb_circle on the same floats)"""
    I, J = np.ascontiguousarray(I), np.ascontiguousarray(J)
    n = len(I)
    si = np.ascontiguousarray(np.broadcast_to(np.asarray(si, np.int32), (n, )))
    sj = np.ascontiguousarray(np.broadcast_to(np.asarray(sj, np.int32), (n, )))
    out, near, ref = np.zeros((n, 4), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib().hx_cr_contacts(I.ctypes.data, si.ctypes.data, J.ctypes.data, sj.ctypes.data, n, out.ctypes.data, near.ctypes.data, ref.ctypes.data)
    return out[:, 0] != 0, out[:, 1], out[:, 2], out[:, 3], near != 0, ref != 0


def put_body(st, slot, x, y, heading=0.0, hl=2.25, hw=0.9, flags=VEH, speed=0.0, velocity=None):
    """A body in `slot`: a vehicle by default; `velocity`: a walker's world-frame velocity (MdDyn.steering / throttle)"""
    sh = st["shape"][slot]
    sh["cx"], sh["cy"], sh["c"], sh["s"], sh["hl"], sh["hw"] = x, y, math.cos(heading), math.sin(heading), hl, hw
    sh["flags"], sh["aux"] = flags, -1
    d = st["dyn"][slot]
    d["heading"], d["speed"] = heading, speed
    d["last_x"], d["last_y"], d["last_c"], d["last_s"] = x - 1.0, y, math.cos(heading), math.sin(heading)
    if velocity is not None:
        d["steering"], d["throttle"] = velocity


def put_barrier(st, slot, x, y, heading=0.0):
    """TrafficBarrier: 2.0 m across the road, 0.3 m along it"""
    put_body(st, slot, x, y, heading, hl=0.15, hw=1.0, flags=abi.KIND_BARRIER | abi.F_ALIVE | abi.F_STATIC)


def put_cone(st, slot, x, y):
    put_body(st, slot, x, y, 0.0, hl=0.2, hw=0.2, flags=abi.KIND_CONE | abi.F_ALIVE | abi.F_STATIC)


def drives(f):
    return ((f & abi.F_ALIVE) != 0) & ((f & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((f & (abi.F_STATIC | abi.F_PENDING)) == 0)


def present(f):
    return ((f & abi.F_ALIVE) != 0) & ((f & abi.KIND_MASK) != abi.KIND_NONE)


KEYS = ("shape", "dyn", "need_reset")


def snapshot(state):
    return {k: state[k].copy() for k in KEYS}


class Coverage:
    """What a rollout showed of the rule, read off the state before and after each md_contact_response: a responder whose cx, cy
    or speed bits changed was resolved; its obstacles (the pair test on the state before) are counted by what they are."""
    def __init__(self):
        self.vehicle_immovable = self.vehicle_vehicle = self.agent_agent = 0
        self.responders = self.resolved = 0

    def note(self, before, after, E, cap):
        sh0, sh1 = before["shape"].reshape(E, cap), after["shape"].reshape(E, cap)
        v0, v1 = before["dyn"]["speed"].reshape(E, cap), after["dyn"]["speed"].reshape(E, cap)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
        moved = (bits(sh0["cx"]) != bits(sh1["cx"])) | (bits(sh0["cy"]) != bits(sh1["cy"])) | (bits(v0) != bits(v1))
        live = (before["need_reset"] == 0)[:, None]
        assert not (moved & ~(drives(sh0["flags"]) & live)).any(), "a slot that is no responder was written"
        self.responders += int((drives(sh0["flags"]) & live).sum())
        self.resolved += int(moved.sum())
        for e, i in zip(*np.nonzero(moved)):
            js = np.nonzero(present(sh0["flags"][e]) & (np.arange(cap) != i))[0]
            hit = contacts(np.repeat(sh0[e, i:i + 1], len(js)), i, sh0[e, js], js)[0]
            assert hit.any(), (e, i)
            for j in js[hit]:
                fj = int(sh0["flags"][e, j])
                if drives(np.int32(fj)):
                    self.vehicle_vehicle += 1
                    self.agent_agent += int(bool(fj & abi.F_AGENT) and bool(int(sh0["flags"][e, i]) & abi.F_AGENT))
                else:
                    self.vehicle_immovable += 1


class ContactOracle:
    """The oracle with the rule in front of every step, as BatchedEngine._step_raw has it; `ped`: md_ped's argument block, applied
    between the rule and the step (tests/ped_host.py)"""
    def __init__(self, host, cr=None, ped=None, state=None):
        import oracle_binding as ob
        self.o = ob.OracleWorld(host, state=state)
        self.host, self.cover, self.ped = host, Coverage(), ped
        self.cr = cr if cr is not None else abi.make_md_contact_response(host.cfg["contact_response_config"])
        self.resets = np.zeros(host.E, np.int64)
        self.crash_vehicle = self.crash_object = 0

    @property
    def state(self):
        return self.o.state

    def _rule(self):
        before = snapshot(self.o.state)
        apply(self.o.state, self.o.k, self.cr)
        self.cover.note(before, self.o.state, self.host.E, self.host.cap)
        self.resets += before["need_reset"] != 0
        if self.ped is not None:
            import ped_host
            ped_host.apply(self.o.state, self.o.k, self.ped)

    def _count(self):
        fl = self.o.state["flags"].reshape(self.host.E, self.host.cap)[:, :self.host.A]
        self.crash_vehicle += int(((fl & abi.FL_CRASH_VEHICLE) != 0).sum())
        self.crash_object += int(((fl & abi.FL_CRASH_OBJECT) != 0).sum())

    def reset(self):
        self.o.state["need_reset"][:] = 1     # BatchedEngine.reset: every env is about to be restored when the rule runs
        self._rule()
        self.o.reset()

    def step(self, actions):
        self._rule()
        self.o.step(actions)
        self._count()
