"""env.render(mode="topdown"): the batched top-down renderer (include/md_render.h; the reference's obs/top_down_renderer.py
TopDownRenderer).  BatchedTopDownRenderer owns md_render's argument block, the picture tensor and the viewer's history on the device;
one render() is one md_render call through the engine's launch path.  The options are checked by check_options(), which needs no
device."""
import ctypes as C

import numpy as np

from metadrive_ped_amd import abi

TOPDOWN_MODES = ("top_down", "topdown", "bev", "birdview")      # envs/base_env.py:490
# the reference's renderer options that are not built: each is refused by name when it is set
REFUSED_OPTIONS = ("semantic_map", "draw_target_vehicle_trajectory", "show_agent_name")


def check_options(num_envs, num_agents, envs=None, screen_size=(512, 512), scaling=5, num_stack=15, history_smooth=0, camera_position=None,
                  target_vehicle_heading_up=False, draw_contour=True, track_agent=0, screen_record=False):
    """-> the options as md_render takes them (a dict that compares equal for equal options); ValueError names what is out of range"""
    ids = [0] if envs is None else [int(e) for e in np.asarray(envs).reshape(-1)]
    if not ids:
        raise ValueError("render: envs is empty")
    for e in ids:
        if not 0 <= e < num_envs:
            raise ValueError("render: envs holds {}, the batch has envs 0 .. {}".format(e, num_envs - 1))
    if len(ids) > 65535:
        raise ValueError("render: at most 65535 envs per call, got {}".format(len(ids)))
    try:
        W, H = (int(v) for v in screen_size)
    except (TypeError, ValueError):
        raise ValueError("render: screen_size must be (width, height), got {!r}".format(screen_size))
    if not (1 <= W <= abi.MD_RD_MAX_SIZE and 1 <= H <= abi.MD_RD_MAX_SIZE):
        raise ValueError("render: screen_size={!r} must lie in [1, {}] on both axes".format(tuple(screen_size), abi.MD_RD_MAX_SIZE))
    scaling = float(scaling)
    if not (scaling > 0.0 and np.isfinite(scaling)):
        raise ValueError("render: scaling={!r} must be positive (pixels per metre)".format(scaling))
    if not 1 <= int(num_stack) <= abi.MD_RD_MAX_STACK:
        raise ValueError("render: num_stack={!r} must lie in [1, {}]".format(num_stack, abi.MD_RD_MAX_STACK))
    if int(history_smooth) < 0:
        raise ValueError("render: history_smooth={!r} must not be negative".format(history_smooth))
    if not 0 <= int(track_agent) < num_agents:
        raise ValueError("render: track_agent={!r} is no agent slot (the envs have {})".format(track_agent, num_agents))
    if camera_position is not None:
        cam = tuple(float(v) for v in np.asarray(camera_position, np.float64).reshape(-1))
        if len(cam) != 2 or not all(np.isfinite(cam)):
            raise ValueError("render: camera_position must be a finite (x, y), got {!r}".format(camera_position))
    else:
        cam = None
    return dict(envs=tuple(ids), screen_size=(W, H), scaling=scaling, num_stack=int(num_stack), history_smooth=int(history_smooth),
                camera_position=cam, target_vehicle_heading_up=bool(target_vehicle_heading_up), draw_contour=bool(draw_contour),
                track_agent=int(track_agent), screen_record=bool(screen_record))


class BatchedTopDownRenderer:
    """The viewer of one batch: `options` is check_options()'s dict.  render() returns the uint8 device tensor [len(envs), H, W, 3]
    (RGB; row 0 is the top of the picture), rewritten by the next call -- .clone() what has to outlive it.  The history (the boxes
    of the last num_stack calls per rendered env) lives in `ring` / `cursor` on the device and empties itself when an env's
    episode clock shows a reset (include/md_render.h); a caller that renders less often than every step can miss one."""
    def __init__(self, engine, options):
        torch = engine.torch
        self.engine, self.options = engine, options
        W, H = options["screen_size"]
        n, S = len(options["envs"]), options["num_stack"]
        self.env_ids = torch.tensor(options["envs"], dtype=torch.int32, device=engine.device)
        self.out = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=engine.device)
        self.ring = torch.zeros((n, S, engine.cap, 8), dtype=torch.int32, device=engine.device)      # MdShape records
        self.cursor = torch.zeros((n, 4), dtype=torch.int32, device=engine.device)
        r = abi.MdRender()
        r.struct_size, r.width, r.height, r.scaling = C.sizeof(abi.MdRender), W, H, options["scaling"]
        r.num_stack, r.history_smooth, r.track_agent = S, options["history_smooth"], options["track_agent"]
        r.heading_up, r.draw_contour = int(options["target_vehicle_heading_up"]), int(options["draw_contour"])
        cam = options["camera_position"]
        r.fixed_camera = int(cam is not None)
        if cam is not None:
            r.cam_x, r.cam_y = cam
        r.n_render = n
        r.env_ids, r.out, r.ring, r.cursor = self.env_ids.data_ptr(), self.out.data_ptr(), self.ring.data_ptr(), self.cursor.data_ptr()
        self._r = r
        self.screen_record = options["screen_record"]
        self.screen_frames = []       # host copies [len(envs), H, W, 3], one per call, only with screen_record

    def render(self):
        eng = self.engine
        with eng._on_device():
            eng._launch("md_render", C.byref(self._r))
        if self.screen_record:
            self.screen_frames.append(self.out.cpu().numpy())
        return self.out

    def history(self):
        """The viewer's history as host numpy copies: ring [n, num_stack, cap] of shape records, cursor [n, 4] (the tests compare them)"""
        return dict(ring=self.ring.cpu().numpy().view(abi.SHAPE_DT).reshape(self.ring.shape[:3]).copy(), cursor=self.cursor.cpu().numpy().copy())

    def generate_gif(self, path="demo.gif", duration=30, env=0):
        """The recorded frames (screen_record=True) of the `env`-th RENDERED env as an animated GIF, `duration` ms per frame
        (TopDownRenderer.generate_gif).  Needs PIL."""
        try:
            from PIL import Image
        except ImportError:
            raise ImportError("generate_gif needs PIL (the Pillow package), which is not installed")
        if not self.screen_frames:
            raise ValueError("generate_gif: no frames recorded; render with screen_record=True")
        imgs = [Image.fromarray(f[env]) for f in self.screen_frames]
        imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=duration, loop=0)
        return path
