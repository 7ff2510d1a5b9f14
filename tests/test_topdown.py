"""The top-down observation's rules (include/md_topdown.h) on their host build, against a float64 numpy restatement written here:
the window transform, point in rotated rectangle, strip about a segment, straight lanes as rectangles and circular lanes as annular
sectors (no cull: every route lane and line piece against every sample).  The restatement also computes how
far every sample lies from every primitive edge; a pixel is compared only where all its samples keep more than 1e-3 m, and there
the float32 image must be equal EXACTLY.  The reference's own numbers (its stack indices, the reset observation, the byte values)
are checked as they are.  This pins the geometry the reference draws, not pygame's pixels."""
import numpy as np
import pytest

import oracle_binding as ob
import topdown_host as th
from metadrive_ped_amd import abi
from metadrive_ped_amd.engine import HostScene
from metadrive_ped_amd.envs import BatchedTopDownMetaDrive

R, DIST, EPS = 84, 30.0, 1e-3
TRAFFIC_F32 = (np.float32(0.299) * np.float32(100) + np.float32(0.587) * np.float32(200) + np.float32(0.114) * np.float32(255)) / np.float32(255)
AHEAD_LEFT = (12.0, 6.0)      # ego frame: forward, left (m)


def _scene():
    """The default single-agent config on map "S" after its reset step; the ego moved to 30 m along its lane, 0.137 m off the
    centre, heading 0.3 rad; slot 1 a vehicle ahead-left, slot 2 one behind-right whose heading (0.02 rad) snaps to 0"""
    cfg = BatchedTopDownMetaDrive(dict(num_envs=1, map="S", build_workers=1)).config
    host = HostScene(cfg)
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
    sh["cx"][0], sh["cy"][0], sh["c"][0], sh["s"][0] = pos[0], pos[1], np.cos(h), np.sin(h)
    ego = np.array([sh["cx"][0], sh["cy"][0]], np.float64)
    fwd, left = np.array([np.cos(h), np.sin(h)]), np.array([-np.sin(h), np.cos(h)])
    for slot, (f, l), hd in ((1, AHEAD_LEFT, 0.45), (2, (-8.0, -3.0), 0.02)):
        p = ego + f * fwd + l * left
        sh["cx"][slot], sh["cy"][slot], sh["c"][slot], sh["s"][slot] = p[0], p[1], np.cos(hd), np.sin(hd)
        sh["hl"][slot], sh["hw"][slot] = 2.2, 0.9
        sh["flags"][slot] = abi.KIND_VEHICLE | abi.F_ALIVE
    return host, st


@pytest.fixture(scope="module")
def scene():
    host, st = _scene()
    img = th.HostTopDown(host).observe(st)
    return host, st, img


def _rect(px, py, cx, cy, ux, uy, s0, s1, half):
    """(inside, near an edge) of the points against the rectangle s0 <= (p - c).u <= s1, |(p - c) x u| <= half, u a unit vector"""
    dx, dy = px - cx, py - cy
    s, lat = dx * ux + dy * uy, dx * uy - dy * ux
    inside = (s >= s0) & (s <= s1) & (np.abs(lat) <= half)
    near = ((np.minimum(np.abs(s - s0), np.abs(s - s1)) < EPS) & (np.abs(lat) <= half + EPS)) | \
           ((np.abs(np.abs(lat) - half) < EPS) & (s >= s0 - EPS) & (s <= s1 + EPS))
    return inside, near


def _sector(px, py, cx, cy, radius, start_phase, dirsign, length, half):
    """(inside, near an edge) of the points against the annular sector of a circular lane, from the geometry: within `half` of the
    circle of `radius` about (cx, cy), at a phase between start_phase and start_phase + dirsign * length / radius.  Near: within
    EPS of either bounding circle or of either end radius"""
    dx, dy = px - cx, py - cy
    rho = np.hypot(dx, dy)
    sweep = length / radius
    assert 0.0 < sweep < 2.0 * np.pi - 0.1 and radius > half
    t = np.mod(dirsign * (np.arctan2(dy, dx) - start_phase), 2.0 * np.pi)      # the phase travelled from the start, in [0, 2 pi)
    inside = (np.abs(rho - radius) <= half) & (t <= sweep)
    tol = EPS / (radius - half)                                                 # EPS of arc at the inner circle, as an angle
    near = (np.minimum(np.abs(rho - (radius - half)), np.abs(rho - (radius + half))) < EPS) & ((t <= sweep + tol) | (t >= 2.0 * np.pi - tol))
    for phi in (start_phase, start_phase + dirsign * sweep):                    # the two end radii, as segments
        ux, uy = np.cos(phi), np.sin(phi)
        along, across = dx * ux + dy * uy, dx * uy - dy * ux
        near |= (np.abs(across) < EPS) & (along >= radius - half - EPS) & (along <= radius + half + EPS)
    return inside, near


def _points(st, fr, fc, R=R, dist=DIST):
    """world points of the image coordinates (fr, fc), float64"""
    sh = st["shape"]
    px, py, hc, hs = (float(sh[k][0]) for k in ("cx", "cy", "c", "s"))
    m = 2.0 * dist / R
    fwd, left = (R / 2.0 - fr) * m, (R / 2.0 - fc) * m
    return px + fwd * hc - left * hs, py + fwd * hs + left * hc


def _restate(host, st, R=R, DIST=DIST, arcs=False):
    """-> road sum4 [R, R], traffic mask [R, R], comparable [R, R], in float64; with arcs also the sub-samples [2R, 2R] on a
    circular route lane and the sub-samples set.  No cull: every route lane and every line piece against every sub-sample"""
    a = host.world.arrays
    sub = (np.arange(2 * R) + 0.5) / 2.0
    x, y = _points(st, sub[:, None], sub[None, :], R, DIST)
    nav = np.zeros(x.shape, bool)
    on_arc = np.zeros(x.shape, bool)
    line = np.zeros(x.shape, bool)
    near = np.zeros(x.shape, bool)
    lanes = a["lanes"][int(a["lane_off"][0]):int(a["lane_off"][1])]
    roads = a["roads"][int(a["road_off"][0]):int(a["road_off"][1])]
    n_route = int(st["nav"]["route_len"][0]) - 1
    for rid in st["route_roads"].reshape(-1, abi.MD_ROUTE_LEN)[0][:n_route]:
        for L in lanes[int(roads[rid]["first_lane"]):int(roads[rid]["first_lane"]) + int(roads[rid]["n_lanes"])]:
            if L["type"] == 0:
                i, n = _rect(x, y, float(L["ax"]), float(L["ay"]), float(L["bx"]), float(L["by"]), 0.0, float(L["length"]), float(L["width"]) / 2.0)
            else:
                assert arcs and L["type"] == 1, "a circular lane in a scene of straight ones"
                i, n = _sector(x, y, float(L["ax"]), float(L["ay"]), float(L["bx"]), float(L["by"]), float(L["dirsign"]), float(L["length"]),
                               float(L["width"]) / 2.0)
                on_arc |= i
            nav |= i
            near |= n
    hw = max(0.3, (2.0 * DIST / R) / 2.0) / 2.0
    quads = a["quads"][int(a["quad_off"][0]):int(a["quad_off"][1])].astype(np.float64)
    kinds = a["quad_kind"][int(a["quad_off"][0]):int(a["quad_off"][1])]
    n_lines = 0
    for q, k in zip(quads, kinds):
        if k not in (abi.Q_LINE_WHITE_CONT, abi.Q_LINE_YELLOW_CONT, abi.Q_LINE_BROKEN):
            continue
        p0, p1 = (q[0:2] + q[6:8]) / 2.0, (q[2:4] + q[4:6]) / 2.0
        ln = np.hypot(*(p1 - p0))
        u = (p1 - p0) / ln
        i, n = _rect(x, y, p0[0], p0[1], u[0], u[1], 0.0, ln, hw)
        line |= i
        near |= n
        n_lines += 1
    assert n_lines > 10
    sum4 = np.where(line, 35, np.where(nav, 64, 0)).reshape(R, 2, R, 2).sum(axis=(1, 3))
    near_px = near.reshape(R, 2, R, 2).any(axis=(1, 3))
    # traffic: pixel centres
    ctr = np.arange(R) + 0.5
    x, y = _points(st, ctr[:, None], ctr[None, :], R, DIST)
    traffic = np.zeros(x.shape, bool)
    sh = st["shape"]
    for j in range(1, host.cap):
        fl = int(sh["flags"][j])
        if not (fl & abi.F_ALIVE) or (fl & abi.KIND_MASK) not in (abi.KIND_VEHICLE, abi.KIND_PEDESTRIAN, abi.KIND_CYCLIST):
            continue
        hd = np.arctan2(float(sh["s"][j]), float(sh["c"][j]))
        hd = hd if abs(hd) > 2 * np.pi / 180 else 0.0
        i, n = _rect(x, y, float(sh["cx"][j]), float(sh["cy"][j]), np.cos(hd), np.sin(hd), -float(sh["hl"][j]), float(sh["hl"][j]), float(sh["hw"][j]))
        traffic |= i
        near_px |= n
    if arcs:
        return sum4, traffic, ~near_px, on_arc, line | nav
    return sum4, traffic, ~near_px


def test_image_equals_the_float64_restatement(scene):
    host, st, img = scene
    sum4, traffic, ok = _restate(host, st)
    assert img.shape == (1, R, R, 5) and img.dtype == np.float32
    assert ok.mean() >= 0.98, ok.mean()
    want_road = np.clip(np.float32(2) * (sum4.astype(np.float32) * np.float32(0.25)) / np.float32(255), 0, 1).astype(np.float32)
    assert len(np.unique(sum4)) > 3 and traffic.sum() > 20
    np.testing.assert_array_equal(img[0, :, :, 0][ok], want_road[ok])
    np.testing.assert_array_equal(img[0, :, :, 2][ok], np.where(traffic, TRAFFIC_F32, np.float32(0))[ok])
    assert 0.0 <= img.min() and img.max() <= 1.0


ARC_SCENES = [(m, h, r, d) for m in ("O", "C", "X") for h in (0.3, np.pi / 2, 2.2) for r, d in ((84, 30.0), (128, 60.0), (33, 20.0))]


def _arc_scene(map_, h, res, dist):
    """The default config on `map_` after its reset step; the ego moved to the middle of the longest circular lane of its route,
    0.137 m off the centre line (outwards), heading h; the two vehicles of _scene around it"""
    cfg = BatchedTopDownMetaDrive(dict(num_envs=1, map=map_, build_workers=1, resolution_size=res, distance=dist)).config
    host = HostScene(cfg)
    o = ob.OracleWorld(host)
    o.reset()
    st = o.state
    a = host.world.arrays
    lanes = a["lanes"][int(a["lane_off"][0]):int(a["lane_off"][1])]
    roads = a["roads"][int(a["road_off"][0]):int(a["road_off"][1])]
    route = st["route_roads"].reshape(-1, abi.MD_ROUTE_LEN)[0][:int(st["nav"]["route_len"][0]) - 1]
    arcs = [L for rid in route for L in lanes[int(roads[rid]["first_lane"]):int(roads[rid]["first_lane"]) + int(roads[rid]["n_lanes"])] if L["type"] == 1]
    assert arcs, "no circular lane on the route of map %r" % map_
    L = max(arcs, key=lambda l: float(l["length"]))
    phi = float(L["by"]) + float(L["dirsign"]) * 0.5 * float(L["length"]) / float(L["bx"])
    rad = float(L["bx"]) + 0.137
    sh = st["shape"]
    sh["cx"][0], sh["cy"][0], sh["c"][0], sh["s"][0] = float(L["ax"]) + rad * np.cos(phi), float(L["ay"]) + rad * np.sin(phi), np.cos(h), np.sin(h)
    ego = np.array([sh["cx"][0], sh["cy"][0]], np.float64)
    fwd, left = np.array([np.cos(h), np.sin(h)]), np.array([-np.sin(h), np.cos(h)])
    for slot, (f, l), hd in ((1, AHEAD_LEFT, 0.45), (2, (-8.0, -3.0), 0.02)):
        p = ego + f * fwd + l * left
        sh["cx"][slot], sh["cy"][slot], sh["c"][slot], sh["s"][slot] = p[0], p[1], np.cos(hd), np.sin(hd)
        sh["hl"][slot], sh["hw"][slot] = 2.2, 0.9
        sh["flags"][slot] = abi.KIND_VEHICLE | abi.F_ALIVE
    sh["flags"][3:] = 0
    return host, st


@pytest.mark.parametrize("map_,h,res,dist", ARC_SCENES, ids=["%s-%.1f-%d" % (m, h, r) for m, h, r, _ in ARC_SCENES])
def test_image_equals_the_float64_restatement_on_arcs(map_, h, res, dist):
    """md_td_on_lane of a circular lane (md_lane_local: md_atan2, md_wrap_to_pi, the nearer end's phase) against the annular sector
    written from the geometry, with the ego mid-arc on a circular route lane.  The host build culls lanes and pieces on their
    bounding boxes, the restatement culls nothing"""
    host, st = _arc_scene(map_, h, res, dist)
    img = th.HostTopDown(host, R=res, distance=dist).observe(st)
    sum4, traffic, ok, on_arc, drawn = _restate(host, st, res, dist, arcs=True)
    assert img.shape == (1, res, res, 5) and img.dtype == np.float32
    assert ok.mean() >= 0.98, ok.mean()
    assert on_arc.sum() >= 200, on_arc.sum()
    partial = drawn.reshape(res, 2, res, 2).sum(axis=(1, 3))
    assert (((partial >= 1) & (partial <= 3)) & ok).sum() >= 10      # partly covered pixels are among the compared ones
    arc_px = on_arc.reshape(res, 2, res, 2).sum(axis=(1, 3))
    assert (((arc_px >= 1) & (arc_px <= 3)) & ok).sum() >= 5         # ... and so are pixels an arc's edge runs through
    want_road = np.clip(np.float32(2) * (sum4.astype(np.float32) * np.float32(0.25)) / np.float32(255), 0, 1).astype(np.float32)
    np.testing.assert_array_equal(img[0, :, :, 0][ok], want_road[ok])
    np.testing.assert_array_equal(img[0, :, :, 2][ok], np.where(traffic, TRAFFIC_F32, np.float32(0))[ok])


def test_orientation_ahead_left_is_upper_left(scene):
    """the ego looks up the image, its left is the image's left: alone in the world, the ahead-left vehicle's blob has its centroid
    within one pixel of the window formula's"""
    host, st, _ = scene
    st = {k: v.copy() for k, v in st.items()}
    st["shape"]["flags"][2:] = 0
    ch = th.HostTopDown(host).observe(st)[0, :, :, 2]
    rows, cols = np.nonzero(ch)
    assert len(rows) > 10
    m = 2 * DIST / R
    want = (R / 2 - AHEAD_LEFT[0] / m - 0.5, R / 2 - AHEAD_LEFT[1] / m - 0.5)
    assert rows.max() < R / 2 and cols.max() < R / 2
    assert abs(rows.mean() - want[0]) <= 1.0 and abs(cols.mean() - want[1]) <= 1.0, (rows.mean(), cols.mean(), want)


def test_reset_observation(scene):
    """_should_fill_stack: every traffic channel is the current frame, past_pos holds exactly one pixel, at (R/2, R/2)"""
    _, st, img = scene
    assert int(st["nav"]["steps"][0]) == 0
    assert img.shape[-1] == 2 + 3
    for ch in (3, 4):
        np.testing.assert_array_equal(img[0, :, :, ch], img[0, :, :, 2])
    rows, cols = np.nonzero(img[0, :, :, 1])
    assert list(zip(rows, cols)) == [(R // 2, R // 2)] and img[0, R // 2, R // 2, 1] == 1.0


def test_stack_indices_are_the_references():
    for length, want in ((1, [0]), (5, [4]), (6, [5, 0]), (11, [10, 5, 0]), (21, [20, 15, 10, 5, 0])):
        assert th.stack_indices(length, 5) == want


def test_past_dot_quirks():
    """scaling = R / distance (twice the window's), clip to +-R, the origin truncated towards zero, outside [0, R) not drawn"""
    lib = th.lib()
    rc = np.zeros(2, np.int32)
    assert lib.hx_past_dot(0.0, 0.0, 0.0, 0.0, 1.0, 0.0, R, DIST, rc.ctypes.data) == 1 and rc.tolist() == [R // 2, R // 2]
    # 5 m behind an ego heading along +x: forward = -5 -> row R/2 + 5 * R / distance = 56
    assert lib.hx_past_dot(-5.0, 0.0, 0.0, 0.0, 1.0, 0.0, R, DIST, rc.ctypes.data) == 1 and rc.tolist() == [56, R // 2]
    # 16 m ahead: row = 42 - 44.8 = -2.8 -> outside; 15.1 m ahead: -0.28 truncates to row 0 and is drawn
    assert lib.hx_past_dot(16.0, 0.0, 0.0, 0.0, 1.0, 0.0, R, DIST, rc.ctypes.data) == 0
    assert lib.hx_past_dot(15.1, 0.0, 0.0, 0.0, 1.0, 0.0, R, DIST, rc.ctypes.data) == 1 and rc[0] == 0
    # far behind: clipped to +R, which lies outside
    assert lib.hx_past_dot(-500.0, 0.0, 0.0, 0.0, 1.0, 0.0, R, DIST, rc.ctypes.data) == 0 and rc[0] == R


def test_history_over_steps():
    """the rings on the host: with no reset in between channel 3 at step t is channel 2 at step t - frame_skip, channel 4 the one at
    t - 2 * frame_skip; the past positions grow as the reference's deque does (the reset step leaves it empty)"""
    cfg = BatchedTopDownMetaDrive(dict(num_envs=1, map="S", build_workers=1, resolution_size=40, traffic_density=0.3)).config
    host = HostScene(cfg)
    o = ob.OracleWorld(host)
    o.reset()
    sh = o.state["shape"]      # a parked vehicle 15 m ahead and 4 m to the left of the start: it moves down the image as the ego drives
    j = host.cap - 1
    sh["cx"][j], sh["cy"][j] = sh["cx"][0] + 15.0 * sh["c"][0] - 4.0 * sh["s"][0], sh["cy"][0] + 15.0 * sh["s"][0] + 4.0 * sh["c"][0]
    sh["c"][j], sh["s"][j], sh["hl"][j], sh["hw"][j] = sh["c"][0], sh["s"][0], 2.2, 0.9
    sh["flags"][j] = abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_STATIC
    td = th.HostTopDown.of_config(host, cfg)
    frames = [td.observe(o.state)]
    for t in range(12):
        o.step(np.tile(np.array([0.0, 1.0], np.float32), (1, 1, 1)))
        frames.append(td.observe(o.state))
    for t in range(1, 13):
        np.testing.assert_array_equal(frames[t][..., 3], frames[max(t - 5, 0)][..., 2])
        np.testing.assert_array_equal(frames[t][..., 4], frames[max(t - 10, 0)][..., 2])
    dots = [int((fr[..., 1] > 0).sum()) for fr in frames]
    # frame t holds min(t, 1) .. positions: one dot up to a deque of 5, at most two up to 10, at most three from 11 on
    assert dots[:6] == [1] * 6 and max(dots[6:11]) == 2 and max(dots[11:]) <= 3, dots
    assert td.hist["cursor"][0].tolist() == [12 % 11, 12 % 21, 12, 0]
    assert any((frames[12][..., 2] != frames[2][..., 2]).ravel())


def test_byte_mode(scene):
    host, st, img = scene
    b = th.HostTopDown(host, norm_pixel=False).observe(st)
    assert b.dtype == np.uint8 and b.shape == img.shape
    assert set(np.unique(b[..., 2])) == {0, 176} and set(np.unique(b[..., 1])) == {0, 255}
    allowed = {2 * ((64 * n1 + 35 * n2) // 4) for n1 in range(5) for n2 in range(5 - n1)}
    assert set(np.unique(b[..., 0])) <= allowed and len(np.unique(b[..., 0])) > 3
    np.testing.assert_array_equal(b[..., 2] > 0, img[..., 2] > 0)
    lib = th.lib()
    assert lib.hx_traffic_byte() == 176 and lib.hx_road_byte(4 * 64) == 128 and lib.hx_road_float(4 * 64) == np.float32(128) / np.float32(255)


def test_config_keys_belong_to_the_top_down_classes():
    from metadrive_ped_amd.envs import (BatchedMetaDriveEnv, BatchedMultiAgentRoundaboutEnv, BatchedTopDownMetaDriveEnvV2,
                                        BatchedTopDownSingleFrameMetaDriveEnv)
    keys = dict(frame_skip=3, frame_stack=2, post_stack=4, norm_pixel=False, resolution_size=33, distance=20)
    for cls, lasers in ((BatchedTopDownMetaDrive, 240), (BatchedTopDownMetaDriveEnvV2, 0)):
        env = cls(dict(keys, num_envs=2))
        assert env.observation_space.shape == (33, 33, 4) and env.observation_space.dtype == np.uint8
        assert env.config["vehicle_config"]["lidar"]["num_lasers"] == lasers
        env = cls(dict(num_envs=2))
        assert env.observation_space.shape == (84, 84, 5) and env.observation_space.dtype == np.float32
        assert {k: cls.default_config()[k] for k in keys} == dict(frame_skip=5, frame_stack=3, post_stack=5, norm_pixel=True,
                                                                  resolution_size=84, distance=30)
    for k, v in keys.items():
        if k == "norm_pixel":      # inert (cosmetic) elsewhere
            BatchedMetaDriveEnv({k: v})
            continue
        with pytest.raises(KeyError):
            BatchedMetaDriveEnv({k: v})
        with pytest.raises(KeyError):
            BatchedMultiAgentRoundaboutEnv({k: v})
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    with pytest.raises(KeyError):
        BatchedScenarioEnv(dict(resolution_size=84))
    with pytest.raises(NotImplementedError, match="multi-agent"):
        BatchedTopDownMetaDrive(dict(num_agents=2))
    with pytest.raises(NotImplementedError, match="TopDownSingleFrameMetaDriveEnv"):
        BatchedTopDownSingleFrameMetaDriveEnv()
    with pytest.raises(ValueError, match="resolution_size"):
        BatchedTopDownMetaDrive(dict(resolution_size=129))
    with pytest.raises(ValueError, match="ring limit"):
        BatchedTopDownMetaDrive(dict(frame_stack=14, frame_skip=5))
    with pytest.raises(TypeError):
        BatchedTopDownMetaDrive(dict(norm_pixel=1))
