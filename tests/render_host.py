"""Host build of include/md_render.h (tests/render_host.c) and a HostRender that plays md_render's part on numpy arrays: the ring,
the cursors and the picture of every rendered env.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import hostlib
from metadrive_ped_amd import abi
from metadrive_ped_amd.engine import make_structs

f, i, P = C.c_float, C.c_int, C.c_void_p


def _declare(lib):
    lib.hx_rd_window.argtypes = [f, f, f, f, i, i, f, f, f, P]
    lib.hx_rd_line_half_width.restype = f
    lib.hx_rd_line_half_width.argtypes = [f]
    lib.hx_rd_drawn_size.argtypes = [i, f, f, P]
    lib.hx_render.restype = None
    lib.hx_render.argtypes = [C.POINTER(abi.MdWorld), C.POINTER(abi.MdState), C.POINTER(abi.MdConfig), C.POINTER(abi.MdRender)]


def lib():
    return hostlib.build("render_host", _declare)


def rgb(packed):
    """0xBBGGRR -> (r, g, b)"""
    return packed & 255, (packed >> 8) & 255, (packed >> 16) & 255


def drawn_size(flags, hl, hw):
    out = np.zeros(2, np.float32)
    lib().hx_rd_drawn_size(flags, hl, hw, out.ctypes.data)
    return float(out[0]), float(out[1])


class HostRender:
    """md_render on the host: render(state) advances the history like one call and returns the pictures [n_render, H, W, 3]"""
    def __init__(self, host, envs=(0, ), screen_size=(512, 512), scaling=5.0, num_stack=15, history_smooth=0, camera_position=None,
                 target_vehicle_heading_up=False, draw_contour=True, track_agent=0):
        self.host = host
        W, H = screen_size
        self.env_ids = np.ascontiguousarray(envs, np.int32)
        n = len(self.env_ids)
        self.out = np.zeros((n, H, W, 3), np.uint8)
        self.hist = dict(ring=np.zeros((n, num_stack, host.cap), abi.SHAPE_DT), cursor=np.zeros((n, 4), np.int32))
        r = abi.MdRender()
        r.struct_size, r.width, r.height, r.scaling = C.sizeof(abi.MdRender), W, H, float(scaling)
        r.num_stack, r.history_smooth, r.track_agent = num_stack, history_smooth, track_agent
        r.heading_up, r.draw_contour, r.fixed_camera = int(target_vehicle_heading_up), int(draw_contour), int(camera_position is not None)
        if camera_position is not None:
            r.cam_x, r.cam_y = float(camera_position[0]), float(camera_position[1])
        r.n_render = n
        self.r = r
        assert lib().hx_sizeof_render() == C.sizeof(abi.MdRender)

    def render(self, state, env_map=None, hist=None):
        """state: the arrays the batch holds (host dtypes); env_map: the maps the envs are on (None: the host scene's); hist: history
        arrays to start from instead of this object's own (they are not modified)"""
        wa = dict(self.host.world.arrays, **self.host.world_scalars())
        if env_map is not None:
            wa["env_map"] = np.ascontiguousarray(env_map, np.int32)
        st = {k: np.ascontiguousarray(v) for k, v in state.items()}
        w, s, k = make_structs(wa, st, self.host.md_config, self.host.world.n_maps, self.host.E, hostlib.ptr)
        if hist is not None:
            self.hist = {k_: np.ascontiguousarray(v).copy() for k_, v in hist.items()}
        self.r.env_ids, self.r.out = self.env_ids.ctypes.data, self.out.ctypes.data
        for name, a in self.hist.items():
            setattr(self.r, name, a.ctypes.data)
        lib().hx_render(C.byref(w), C.byref(s), C.byref(k), C.byref(self.r))
        return self.out.copy()
