"""ctypes binding of tests/ai_protect_host.c, the host build of include/md_ai_protect.h (compiled on first use into a temporary
directory by tests/hostlib.py).  TEST INFRASTRUCTURE."""
import ctypes as C
import os

import numpy as np

import hostlib
from hostlib import ptr as _p

from metadrive_ped_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ai_protect.npz")
# MdProtectIn
IN_DT = np.dtype([(k, np.float32) for k in ("obs0", "obs1", "heading_diff", "speed_kmh", "max_speed_kmh", "lat_min", "lon_min")])
TAKEOVER, TAKEOVER_START, TAKEOVER_END = abi.AIP_TAKEOVER, abi.AIP_TAKEOVER_START, abi.AIP_TAKEOVER_END


def _declare(L):
    P = C.c_void_p
    L.hx_heading_diff.argtypes = [P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]
    L.hx_heading_diff.restype = C.c_float
    L.hx_windows.argtypes = [P, C.c_int, P, P]
    L.hx_act.argtypes = [C.c_int] + [P] * 8
    L.hx_batch.argtypes = [P] * 9 + [C.POINTER(abi.MdConfig), P, P, C.c_float] + [P] * 5


def lib():
    return hostlib.build("ai_protect_host", _declare)


def lane_record(kind, **f):
    """One MdLane: kind "straight" (sx, sy, ex, ey) or "circular" (ax, ay = the centre, dirsign = +1 counter-clockwise / -1)."""
    L = np.zeros(1, abi.LANE_DT)
    L["type"] = 0 if kind == "straight" else 1
    for k, v in f.items():
        L[k] = v
    return L


def heading_diff(lanes, lane, x, y, hc, hs):
    return float(lib().hx_heading_diff(_p(lanes), int(lane), x, y, hc, hs))


def windows(cloud):
    cloud = np.ascontiguousarray(cloud, np.float32)
    lat, lon = C.c_float(), C.c_float()
    lib().hx_windows(_p(cloud), cloud.size, C.addressof(lat), C.addressof(lon))
    return lat.value, lon.value


def act(raw, sv, inputs, save_level, expert_takeover, takeover):
    """n independent calls -> (applied [n, 2], flags [n] uint8, takeover after [n] uint8); `inputs`: IN_DT [n]"""
    raw, sv = np.ascontiguousarray(raw, np.float32).reshape(-1, 2), np.ascontiguousarray(sv, np.float32).reshape(-1, 2)
    n = len(raw)
    inputs = np.ascontiguousarray(inputs, IN_DT)
    sl = np.ascontiguousarray(np.broadcast_to(np.asarray(save_level, np.float32), (n, )))
    et = np.ascontiguousarray(np.broadcast_to(np.asarray(expert_takeover, np.uint8), (n, )))
    tk = np.array(np.broadcast_to(np.asarray(takeover, np.uint8), (n, )))
    applied, flags = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    lib().hx_act(n, _p(raw), _p(sv), _p(inputs), _p(sl), _p(et), _p(tk), _p(applied), _p(flags))
    return applied, flags, tk


def batch(world, state, md_config, obs, raw, sv, save_level, takeover, expert_takeover):
    """md_ai_protect restated on host arrays: world = the WorldTables arrays, state = the (downloaded) state dict, obs [E, obs_dim].
    takeover / expert_takeover [E] uint8 are updated in place.  -> (applied [E, 2], flags [E], the saver's inputs IN_DT [E])"""
    E = md_config.n_envs
    raw, sv = np.ascontiguousarray(raw, np.float32).reshape(E, 2), np.ascontiguousarray(sv, np.float32).reshape(E, 2)
    obs = np.ascontiguousarray(obs, np.float32).reshape(E, md_config.obs_dim)
    applied, flags, ins = np.zeros((E, 2), np.float32), np.zeros(E, np.uint8), np.zeros(E, IN_DT)
    c = lambda a: np.ascontiguousarray(a)
    args = [c(world["lanes"]), c(world["lane_off"]), c(world["env_map"]), c(state["shape"]), c(state["dyn"]), c(state["param"]),
            c(state["nav"]), obs, c(state["need_reset"])]
    lib().hx_batch(*[_p(a) for a in args], C.byref(md_config), _p(raw), _p(sv), float(save_level), _p(takeover), _p(expert_takeover),
                   _p(applied), _p(flags), _p(ins))
    return applied, flags, ins
