"""The top-down renderer's rules (include/md_render.h) on their host build (tests/render_host.c), against a float64 numpy
restatement written here: the window transform, the strips of the line pieces, the boxes of three held frames painted in the
painter's order, the fade and the contour.  The restatement also computes how far every pixel centre lies from every primitive
edge; a pixel is compared only where it keeps more than 1e-3 m, and there the RGB bytes must be equal EXACTLY.  At most 1 % of the
pixels may be left out: the bands' area is edge length x 2e-3 m, under 0.1 % of a 100 m window at 0.2 - 0.5 m pixels.  The
reference's own numbers (colours, fade bytes, the history_smooth pattern, the drawn sizes) are checked as they are.  This pins the
geometry the reference draws, not pygame's pixels."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_binding as ob
import render_host as rh
from metadrive_ped_amd import abi
from metadrive_ped_amd.engine import HostScene
from metadrive_ped_amd.envs import BatchedMetaDriveEnv

EPS = 1e-3
W, H, SCALING = 250, 200, 2.5          # a 100 m x 80 m window at 0.4 m pixels
GREEN, PROP, CONTOUR, WHITE = (2, 158, 115), (235, 84, 42), (60, 60, 60), (255, 255, 255)
LINE_RGB = {abi.Q_LINE_YELLOW_CONT: (255, 175, 35), abi.Q_LINE_BROKEN: (175, 175, 175), abi.Q_LINE_WHITE_CONT: (95, 95, 95)}
LINE_ORDER = {abi.Q_LINE_BROKEN: 1, abi.Q_LINE_WHITE_CONT: 2, abi.Q_LINE_YELLOW_CONT: 3}
# sns.color_palette("colorblind") as bytes, entry 2 (the agents' green) taken out
PALETTE = [(1, 115, 178), (222, 143, 5), (213, 94, 0), (204, 120, 188), (202, 145, 97), (251, 175, 228), (148, 148, 148), (236, 225, 51),
           (86, 180, 233)]
PROPS = (abi.KIND_CONE, abi.KIND_WARNING, abi.KIND_BARRIER)
# slot -> (forward, left of the ego at frame 0, heading, hl, hw, flags); slots 3 and 4 overlap
MOVERS = {1: (12.0, 6.0, 0.45, 2.2, 0.9, abi.KIND_VEHICLE | abi.F_ALIVE),
          2: (-8.0, -3.0, 0.02, 2.2, 0.9, abi.KIND_VEHICLE | abi.F_ALIVE),              # 0.02 rad snaps to 0
          3: (20.0, -5.0, 0.9, 2.4, 1.0, abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_STATIC),      # two broken-down vehicles
          4: (21.0, -4.5, 0.2, 2.4, 1.0, abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_STATIC),
          5: (6.0, 3.0, 0.7, 0.2, 0.2, abi.KIND_CONE | abi.F_ALIVE | abi.F_STATIC),
          6: (-3.0, 5.0, 1.2, 0.35, 0.35, abi.KIND_PEDESTRIAN | abi.F_ALIVE)}
ADVANCE = 3.0      # metres every non-static mover moves along its heading between two frames


def _frames():
    """The default single-agent config on map "S" after its reset step; the ego moved to 30 m along its lane, heading 0.3 rad, and
    the movers of MOVERS around it; three frames, every non-static mover ADVANCE metres further along its heading in each, the
    episode clock (MdNav.steps of slot 0) 1, 2, 3 -> [state of frame 0, 1, 2]"""
    cfg = BatchedMetaDriveEnv(dict(num_envs=1, map="S", build_workers=1)).config
    host = HostScene(cfg)
    assert host.cap > max(MOVERS)
    o = ob.OracleWorld(host)
    o.reset()
    st = o.state
    a = host.world.arrays
    lane = a["lanes"][int(a["lane_off"][0]) + int(st["nav"]["lane"][0])]
    assert lane["type"] == 0
    d = np.array([lane["bx"], lane["by"]], np.float64)
    pos = np.array([lane["ax"], lane["ay"]], np.float64) + 30.0 * d + 0.137 * np.array([d[1], -d[0]])
    h = 0.3
    sh = st["shape"]
    sh["flags"][1:] = 0
    sh["cx"][0], sh["cy"][0], sh["c"][0], sh["s"][0] = pos[0], pos[1], np.cos(h), np.sin(h)
    assert int(sh["flags"][0]) & abi.F_AGENT
    fwd, left = np.array([np.cos(h), np.sin(h)]), np.array([-np.sin(h), np.cos(h)])
    for slot, (f, l, hd, hl, hw, fl) in MOVERS.items():
        p = pos + f * fwd + l * left
        sh["cx"][slot], sh["cy"][slot], sh["c"][slot], sh["s"][slot] = p[0], p[1], np.cos(hd), np.sin(hd)
        sh["hl"][slot], sh["hw"][slot], sh["flags"][slot] = hl, hw, fl
    frames = []
    for k in range(3):
        f = {name: v.copy() for name, v in st.items()}
        s2 = f["shape"]
        move = (s2["flags"] & abi.F_STATIC) == 0
        s2["cx"][move] += np.float32(ADVANCE * k) * s2["c"][move]
        s2["cy"][move] += np.float32(ADVANCE * k) * s2["s"][move]
        f["nav"]["steps"][0] = k + 1
        frames.append(f)
    return host, frames


@pytest.fixture(scope="module")
def scene():
    return _frames()


def _render(host, frames, **opts):
    r = rh.HostRender(host, screen_size=(W, H), scaling=SCALING, **opts)
    imgs = [r.render(f) for f in frames]
    return r, imgs


def _rect(px, py, cx, cy, ux, uy, s0, s1, half):
    """(inside, near an edge) of the points against the rectangle s0 <= (p - c).u <= s1, |(p - c) x u| <= half, u a unit vector"""
    dx, dy = px - cx, py - cy
    s, lat = dx * ux + dy * uy, dx * uy - dy * ux
    inside = (s >= s0) & (s <= s1) & (np.abs(lat) <= half)
    near = ((np.minimum(np.abs(s - s0), np.abs(s - s1)) < EPS) & (np.abs(lat) <= half + EPS)) | \
           ((np.abs(np.abs(lat) - half) < EPS) & (s >= s0 - EPS) & (s <= s1 + EPS))
    return inside, near, s, lat


def _drawn(kind, hl, hw):
    """top_down_length / 2, top_down_width / 2 by kind, from the reference's classes"""
    return {abi.KIND_CONE: (4 * 0.2 / 2, 4 * 0.2 / 2), abi.KIND_WARNING: (2 * 0.5 / 2, 2 * 0.5 / 2), abi.KIND_BARRIER: (2 * 0.3 / 2, 2.0 / 2),
            abi.KIND_PEDESTRIAN: (2 * 0.35 / 2, 2 * 0.35 / 2), abi.KIND_BUILDING: (10 / 2, 3 / 2)}.get(kind, (hl, hw))


def _fade(c, n, k):
    """the header's float32 rule, restated with numpy's float32"""
    alpha = np.float32(0) if k == n - 1 else np.float32(n - k) / np.float32(n)
    return tuple(int(np.float32(v) + alpha * np.float32(255 - v)) for v in c)


def _restate(host, frames, heading_up=False, camera=None, smooth=0, contour=True):
    """-> (image [H, W, 3] uint8, comparable [H, W]) of the LAST frame with the earlier ones as its history, in float64"""
    a = host.world.arrays
    cur = frames[-1]["shape"]
    px, py = (float(cur["cx"][0]), float(cur["cy"][0])) if (camera is None or heading_up) else camera
    uc, us = (float(cur["c"][0]), float(cur["s"][0])) if heading_up else (0.0, 1.0)
    up = (H / 2.0 - (np.arange(H) + 0.5))[:, None] / SCALING
    right = ((np.arange(W) + 0.5) - W / 2.0)[None, :] / SCALING
    x, y = px + up * uc + right * us, py + up * us - right * uc
    img = np.empty((H, W, 3), np.uint8)
    img[:] = WHITE
    near = np.zeros((H, W), bool)
    hw = max(0.3, 1.0 / SCALING) / 2.0
    quads = a["quads"][int(a["quad_off"][0]):int(a["quad_off"][1])].astype(np.float64)
    kinds = a["quad_kind"][int(a["quad_off"][0]):int(a["quad_off"][1])]
    order = np.zeros((H, W), int)
    for q, k in zip(quads, kinds):
        if int(k) not in LINE_ORDER:
            continue
        p0, p1 = (q[0:2] + q[6:8]) / 2.0, (q[2:4] + q[4:6]) / 2.0
        ln = np.hypot(*(p1 - p0))
        u = (p1 - p0) / ln
        i, n, _, _ = _rect(x, y, p0[0], p0[1], u[0], u[1], 0.0, ln, hw)
        order = np.where(i, np.maximum(order, LINE_ORDER[int(k)]), order)
        near |= n
    for k, o in LINE_ORDER.items():
        img[order == o] = LINE_RGB[k]
    assert len(np.unique(order)) >= 3
    n_held = len(frames)
    cw = 2.0 / SCALING
    for k, f in enumerate(frames):
        if k < n_held - 1 and smooth != 0 and (n_held - k) % smooth != 0:
            continue
        sh = f["shape"]
        for j in range(host.cap):
            fl = int(sh["flags"][j])
            if not (fl & abi.F_ALIVE) or (fl & abi.KIND_MASK) == abi.KIND_NONE:
                continue
            hd = np.arctan2(float(sh["s"][j]), float(sh["c"][j]))
            hd = hd if abs(hd) > 2 * np.pi / 180 else 0.0
            hl, hw_ = _drawn(fl & abi.KIND_MASK, float(sh["hl"][j]), float(sh["hw"][j]))
            i, n, s, lat = _rect(x, y, float(sh["cx"][j]), float(sh["cy"][j]), np.cos(hd), np.sin(hd), -hl, hl, hw_)
            base = GREEN if fl & abi.F_AGENT else (PROP if (fl & abi.KIND_MASK) in PROPS else PALETTE[j % 9])
            img[i] = _fade(base, n_held, k)
            near |= n
            if k == n_held - 1 and contour:
                edge = i & ((hl - np.abs(s) < cw) | (hw_ - np.abs(lat) < cw))
                img[edge] = CONTOUR
                near |= i & ((np.abs(hl - np.abs(s) - cw) < EPS) | (np.abs(hw_ - np.abs(lat) - cw) < EPS))
    return img, ~near


CASES = {"world_axes": dict(), "heading_up": dict(target_vehicle_heading_up=True, history_smooth=2),
         "fixed_camera": dict(camera_position="ahead", draw_contour=False)}


@pytest.mark.parametrize("case", list(CASES))
def test_image_equals_the_float64_restatement(scene, case):
    host, frames = scene
    opts = dict(CASES[case])
    if opts.get("camera_position") == "ahead":      # 10 m east, 5 m north of the ego's last position
        opts["camera_position"] = (float(frames[-1]["shape"]["cx"][0]) + 10.0, float(frames[-1]["shape"]["cy"][0]) + 5.0)
    r, imgs = _render(host, frames, **opts)
    assert imgs[-1].shape == (1, H, W, 3) and imgs[-1].dtype == np.uint8
    assert r.hist["cursor"][0].tolist() == [2, 3, 3, 0]
    want, ok = _restate(host, frames, heading_up=opts.get("target_vehicle_heading_up", False), camera=opts.get("camera_position"),
                        smooth=opts.get("history_smooth", 0), contour=opts.get("draw_contour", True))
    left_out = 1.0 - ok.mean()
    print("%s: %.4f %% of the pixels lie within 1e-3 m of an edge" % (case, 100 * left_out))
    assert left_out <= 0.01, left_out
    got = imgs[-1][0]
    bad = np.argwhere((got != want).any(-1) & ok)
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    colours = {tuple(c) for c in np.unique(got.reshape(-1, 3), axis=0)}
    assert {WHITE, PALETTE[1]} <= colours and len(set(LINE_RGB.values()) & colours) >= 2
    # the cone (0.8 m) and the pedestrian (0.7 m) are narrower than two contours of 2 pixels = 0.8 m: all contour where one is drawn
    # (and of the ego's 1.8 m a strip of 0.2 m stays green, which may hold no pixel centre)
    if opts.get("draw_contour", True):
        assert CONTOUR in colours and not {PROP, PALETTE[6]} & colours
    else:
        assert CONTOUR not in colours and {GREEN, PROP, PALETTE[6]} <= colours
    assert _fade(GREEN, 3, 1) in colours      # the ego's box of one frame ago


def _pixel_of(cam, pt, up_vec=(0.0, 1.0)):
    """(row, col) of the pixel that holds the world point pt"""
    dx, dy = pt[0] - cam[0], pt[1] - cam[1]
    up, right = dx * up_vec[0] + dy * up_vec[1], dx * up_vec[1] - dy * up_vec[0]
    return int(np.floor(H / 2.0 - up * SCALING)), int(np.floor(W / 2.0 + right * SCALING))


def test_orientations(scene):
    """world x to the right and world y up by default; heading up, the tracked agent looks up the image; a fixed camera sits at
    the image's centre"""
    host, frames = scene
    sh = frames[-1]["shape"]
    ego = (float(sh["cx"][0]), float(sh["cy"][0]))
    ahead = (ego[0] + 1.5 * float(sh["c"][0]), ego[1] + 1.5 * float(sh["s"][0]))      # inside the ego's box, clear of the contour
    _, imgs = _render(host, frames[-1:], draw_contour=False)
    row, col = _pixel_of(ego, ahead)
    assert tuple(imgs[0][0, row, col]) == GREEN and col > W // 2 and row < H // 2      # heading 0.3 rad: right of and above the centre
    assert tuple(imgs[0][0, H // 2, W // 2]) == GREEN
    _, imgs = _render(host, frames[-1:], target_vehicle_heading_up=True, draw_contour=False)
    assert tuple(imgs[0][0, H // 2 - 4, W // 2]) == GREEN and tuple(imgs[0][0, H // 2, W // 2 + 4]) != GREEN      # 1.6 m ahead; 1.6 m to the right
    cam = (ego[0] + 10.0, ego[1] + 5.0)
    _, imgs = _render(host, frames[-1:], camera_position=cam, draw_contour=False)
    row, col = _pixel_of(cam, ahead)
    assert tuple(imgs[0][0, row, col]) == GREEN and col < W // 2 and row > H // 2
    # heading up, the camera is the tracked agent whatever camera_position says (top_down_renderer.py:505-506)
    _, both = _render(host, frames[-1:], target_vehicle_heading_up=True, camera_position=cam)
    _, up = _render(host, frames[-1:], target_vehicle_heading_up=True)
    assert np.array_equal(both[0], up[0])


def test_slot_order_decides_where_boxes_overlap(scene):
    host, frames = scene
    sh = frames[-1]["shape"]
    c4 = (float(sh["cx"][4]), float(sh["cy"][4]))
    d = (c4[0] - float(sh["cx"][3]), c4[1] - float(sh["cy"][3]))
    along, across = d[0] * sh["c"][3] + d[1] * sh["s"][3], d[1] * sh["c"][3] - d[0] * sh["s"][3]
    assert abs(along) < 2.4 and abs(across) < 1.0          # slot 4's centre lies inside slot 3's box
    _, imgs = _render(host, frames[-1:], draw_contour=False)
    ego = (float(sh["cx"][0]), float(sh["cy"][0]))
    row, col = _pixel_of(ego, c4)
    assert tuple(imgs[0][0, row, col]) == PALETTE[4]
    c3 = (float(sh["cx"][3]) - 1.2 * float(sh["c"][3]), float(sh["cy"][3]) - 1.2 * float(sh["s"][3]))      # slot 3's rear half, outside slot 4
    row, col = _pixel_of(ego, c3)
    assert tuple(imgs[0][0, row, col]) == PALETTE[3]


def test_the_references_colours():
    lib = rh.lib()
    for kind, want in LINE_RGB.items():
        assert rh.rgb(lib.hx_rd_line_rgb(kind)) == want
    assert [lib.hx_rd_line_order(k) for k in (abi.Q_LINE_BROKEN, abi.Q_LINE_WHITE_CONT, abi.Q_LINE_YELLOW_CONT)] == [1, 2, 3]
    assert lib.hx_rd_line_order(abi.Q_SIDEWALK) == 0 and lib.hx_rd_line_order(abi.Q_CROSSWALK) == 0
    assert rh.rgb(lib.hx_rd_base_rgb(abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT, 7)) == GREEN
    for kind in PROPS:
        assert rh.rgb(lib.hx_rd_base_rgb(kind | abi.F_ALIVE | abi.F_STATIC, 5)) == PROP
    for slot in range(20):
        for kind in (abi.KIND_VEHICLE, abi.KIND_PEDESTRIAN, abi.KIND_CYCLIST, abi.KIND_BUILDING):
            assert rh.rgb(lib.hx_rd_base_rgb(kind | abi.F_ALIVE, slot)) == PALETTE[slot % 9]
    assert GREEN not in PALETTE and len(set(PALETTE)) == 9
    assert rh.rgb(lib.hx_rd_contour_rgb()) == CONTOUR


def test_fade_bytes():
    """c + alpha * (255 - c) truncated, alpha = i / n with i = n - k (top_down_renderer.py:417-433): for n = 3 the exact values"""
    lib = rh.lib()
    for c in (GREEN, PROP) + tuple(PALETTE):
        packed = c[0] | (c[1] << 8) | (c[2] << 16)
        for k in (0, 1):
            want = tuple(int(v + Fraction(3 - k, 3) * (255 - v)) for v in c)
            assert rh.rgb(lib.hx_rd_fade(packed, 3, k)) == want, (c, k)
        assert rh.rgb(lib.hx_rd_fade(packed, 3, 2)) == c          # the current frame: alpha 0
        assert rh.rgb(lib.hx_rd_fade(packed, 3, 0)) == WHITE      # the oldest of three: alpha 1
    assert rh.rgb(lib.hx_rd_fade(GREEN[0] | (GREEN[1] << 8) | (GREEN[2] << 16), 3, 1)) == (170, 222, 208)


def test_history_smooth_skip_pattern():
    """frame k of n is skipped when (n - k) % history_smooth != 0; never the current one"""
    lib = rh.lib()
    assert [lib.hx_rd_frame_skipped(6, k, 2) for k in range(6)] == [0, 1, 0, 1, 0, 0]
    assert [lib.hx_rd_frame_skipped(7, k, 3) for k in range(7)] == [1, 0, 1, 1, 0, 1, 0]
    assert [lib.hx_rd_frame_skipped(5, k, 0) for k in range(5)] == [0] * 5
    assert [lib.hx_rd_frame_skipped(5, k, 1) for k in range(5)] == [0] * 5


def test_drawn_sizes_per_kind():
    A = abi.F_ALIVE
    assert rh.drawn_size(abi.KIND_VEHICLE | A, 2.2, 0.9) == (np.float32(2.2), np.float32(0.9))
    assert rh.drawn_size(abi.KIND_CYCLIST | A, 0.875, 0.2) == (np.float32(0.875), np.float32(0.2))
    assert rh.drawn_size(abi.KIND_CONE | A, 0.2, 0.2) == (np.float32(0.4), np.float32(0.4))              # 4 * RADIUS square
    assert rh.drawn_size(abi.KIND_WARNING | A, 0.5, 0.5) == (0.5, 0.5)                                    # 2 * RADIUS square
    assert rh.drawn_size(abi.KIND_BARRIER | A, 0.15, 1.0) == (np.float32(0.3), 1.0)                       # 2 * WIDTH x LENGTH
    assert rh.drawn_size(abi.KIND_PEDESTRIAN | A, 0.35, 0.35) == (np.float32(0.35), np.float32(0.35))     # 2 * RADIUS square
    assert rh.drawn_size(abi.KIND_BUILDING | A, 5.0, 1.75) == (5.0, 1.5)                                  # BUILDING_LENGTH x 3
    assert rh.lib().hx_rd_line_half_width(5.0) == np.float32(0.15) and rh.lib().hx_rd_line_half_width(0.5) == 1.0


def test_history_is_emptied_by_the_episode_clock(scene):
    """the clock 0, or smaller than at the previous call, starts the history again; otherwise it grows to num_stack and turns"""
    host, frames = scene
    r = rh.HostRender(host, screen_size=(32, 32), scaling=1.0, num_stack=2)
    f = {k: v.copy() for k, v in frames[0].items()}
    seen = []
    for clock in (0, 1, 2, 3, 1, 2, 0, 0, 5):
        f["nav"]["steps"][0] = clock
        r.render(f)
        seen.append(r.hist["cursor"][0].tolist())
    assert seen == [[0, 1, 0, 0], [1, 2, 1, 0], [0, 2, 2, 0], [1, 2, 3, 0], [0, 1, 1, 0], [1, 2, 2, 0], [0, 1, 0, 0], [0, 1, 0, 0], [1, 2, 5, 0]]
