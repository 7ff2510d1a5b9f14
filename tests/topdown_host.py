"""Host build of include/md_topdown.h (tests/topdown_host.c) and a HostTopDown that plays md_topdown's part on numpy arrays: the
rings, the cursors and the image of every env.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
from metadrive_ped_amd import abi
from metadrive_ped_amd.engine import make_structs

f, i, P = C.c_float, C.c_int, C.c_void_p


def _declare(lib):
    lib.hx_window.argtypes = [f, f, f, f, i, f, f, f, P]
    lib.hx_stack_indices.argtypes = [i, i, P]
    lib.hx_past_dot.argtypes = [f, f, f, f, f, f, i, f, P]
    lib.hx_line_half_width.restype = f
    lib.hx_line_half_width.argtypes = [i, f]
    lib.hx_road_float.restype = f
    lib.hx_road_float.argtypes = [i]
    lib.hx_road_byte.argtypes = [i]
    lib.hx_traffic_float.restype = f
    lib.hx_topdown.restype = None
    lib.hx_topdown.argtypes = [C.POINTER(abi.MdWorld), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdTopDown)]


def lib():
    return hostlib.build("topdown_host", _declare)


def stack_indices(length, skip):
    out = np.zeros(128, np.int32)
    n = lib().hx_stack_indices(length, skip, out.ctypes.data)
    return out[:n].tolist()


class HostTopDown:
    """md_topdown on the host: observe(state) advances the history like one launch and returns the image [E, R, R, C]"""
    def __init__(self, host, R=84, distance=30.0, frame_stack=3, frame_skip=5, post_stack=5, norm_pixel=True):
        self.host, self.R, self.C = host, R, 2 + frame_stack
        Lt, Lp = abi.td_ring_len(frame_stack, frame_skip), abi.td_ring_len(post_stack, frame_skip)
        self.out = np.zeros((host.E, R, R, self.C), np.float32 if norm_pixel else np.uint8)
        self.hist = dict(ring_traffic=np.zeros((host.E, Lt, R, abi.td_row_words(R)), np.int32),
                         ring_pos=np.zeros((host.E, Lp, 2), np.float32), cursor=np.zeros((host.E, 4), np.int32))
        td = abi.MdTopDown()
        td.struct_size, td.resolution, td.distance = C.sizeof(abi.MdTopDown), R, float(distance)
        td.frame_stack, td.frame_skip, td.post_stack, td.norm_pixel = frame_stack, frame_skip, post_stack, int(norm_pixel)
        self.td = td
        assert lib().hx_sizeof_topdown() == C.sizeof(abi.MdTopDown)

    @classmethod
    def of_config(cls, host, cfg):
        return cls(host, cfg["resolution_size"], cfg["distance"], cfg["frame_stack"], cfg["frame_skip"], cfg["post_stack"], cfg["norm_pixel"])

    def observe(self, state, env_map=None, hist=None):
        """state: the arrays md_step left (host dtypes); env_map: the maps the envs were on in that step (None: the host scene's);
        hist: history arrays to start from instead of this object's own (they are not modified)"""
        wa = dict(self.host.world.arrays, **self.host.world_scalars())
        if env_map is not None:
            wa["env_map"] = np.ascontiguousarray(env_map, np.int32)
        st = {k: np.ascontiguousarray(v) for k, v in state.items()}
        w, s, k = make_structs(wa, st, self.host.md_config, self.host.world.n_maps, self.host.E, hostlib.ptr)
        if hist is not None:
            self.hist = {k_: np.ascontiguousarray(v).copy() for k_, v in hist.items()}
        self.td.out = self.out.ctypes.data
        for name, a in self.hist.items():
            setattr(self.td, name, a.ctypes.data)
        lib().hx_topdown(C.byref(w), C.byref(s), C.byref(k), C.byref(self.td))
        return self.out.copy()
