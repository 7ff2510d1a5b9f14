"""Host side of SCENARIO mode: scenario descriptions (the reference's unified format, metadrive/scenario/
scenario_description.py) -> the tables and reset state of a batch of ScenarioEnv scenes.

What the reference does per episode (envs/scenario_env.py, manager/scenario_map_manager.py:49-75,
manager/scenario_traffic_manager.py, manager/scenario_data_manager.py) and what becomes of it here:

  ScenarioMapManager.update_route   the SDC's recorded track -> PointLane reference trajectory, the agent's spawn pose /
                                    velocity = the track's first frame            -> slot 0, polyline 0, checkpoint table
  ScenarioTrafficManager            every other track -> a mover slot: frames [T] of pose / validity (replay), its own
                                    path as a polyline + outline polygon (TrajectoryIDMPolicy route), static / length tests
  TrajectoryNavigation.set_route    checkpoints every 2 m along the reference trajectory

PolyLine restates utils/interpolating_line.py:12-71 (segment construction) in float64; the device tables are float32.
Road lines and road boundaries of a description's `map_features` ARE bodies (line pieces in the scene's own static map: the
side / lane-line detectors see them, crossing them raises the line flags; pinned by tests/golden/scenario_lines.json).  A
description without such features -- e.g. the lanes-only maps scenario_export.py writes -- simply has none: the side detector
then reports "nothing" and no line flag is raised.  Sidewalk / crosswalk polygons are not built.
"""
import copy
import math
import os

import numpy as np

from metadrive_ped_amd import abi
from metadrive_ped_amd.mapgen.tables import beam_table
from metadrive_ped_amd.obs_layout import ObsLayout
from metadrive_ped_amd.scene import HostSceneBase, step_state

# ScenarioEnv's own defaults (envs/scenario_env.py:21-95); keys not listed keep BaseEnv's
SCENARIO_DEFAULT_CONFIG = dict(
    data_directory=None,          # a ScenarioNet dataset folder (scenario_data.py); None: descriptions are handed in / synthetic
    start_scenario_index=0, num_scenarios=3, sequential_seed=False,
    no_traffic=False, no_static_vehicles=False, no_light=False, reactive_traffic=False, filter_overlapping_car=True,
    even_sample_vehicle_class=True, default_vehicle_in_traffic=False, static_traffic_object=True,
    success_reward=5.0, out_of_road_penalty=5.0, on_lane_line_penalty=1.0, crash_vehicle_penalty=1.0,
    crash_object_penalty=1.0, crash_human_penalty=1.0, driving_reward=1.0, steering_range_penalty=0.5,
    heading_penalty=1.0, lateral_penalty=0.5, max_lateral_dist=4.0, no_negative_reward=True,
    crash_vehicle_cost=1.0, crash_object_cost=1.0, out_of_road_cost=1.0, crash_human_cost=1.0,
    out_of_route_done=False, crash_vehicle_done=False, crash_object_done=False, crash_human_done=False,
    relax_out_of_road_done=True, allowed_more_steps=None,
    map_region_size=512,          # envs/scenario_env.py:40: line bodies exist within +-256 m of the origin
    # the scenario walk (no key of the reference's: its ScenarioEnv picks a new scenario at every reset by itself): True = every
    # env moves on to another scenario of [start_scenario_index, + num_scenarios) whenever its episode ends (walk_scene)
    walk_scenarios=False,
    walk_stride=None,             # W, the envs over all shards (sharding.shard_config sets it); None: num_envs
    scenario_pool_max_bytes=64 << 30,   # a walk's scene pool larger than this (device bytes) is refused
    # ScenarioEnv's curriculum (envs/scenario_env.py:31-33), per env of a walk (include/md_curriculum.h, curriculum_params)
    curriculum_level=1, episodes_to_evaluate_curriculum=None, target_success_rate=0.8,
    # the vector scene observation of scenario mode (include/md_scenario_vector_obs.h; no key of the reference's): None = off, no
    # launch and no array; a dict (an empty one too) is laid over config.SCENARIO_VECTOR_OBS_DEFAULT_CONFIG and env.vector_obs()
    # returns the blocks
    scenario_vector_obs=None,
    # the traffic lights of a description's dynamic_map_states (include/md_traffic_lights.h; the reference's ScenarioLightManager,
    # which it registers unless no_light): None = off, no table, no launch and no info key -- NOT the reference's default, so that a
    # batch behaves as it did before the lights were built; a dict (an empty one too) is laid over
    # config.TRAFFIC_LIGHTS_DEFAULT_CONFIG.  skip_missing_light (envs/scenario_env.py:51) is read only with the key set.
    traffic_lights=None, skip_missing_light=True,
    # the closed-loop driving metrics (include/md_scenario_metrics.h; no key of the reference's): None = off, no launch, no array and
    # no info key; a dict (an empty one too) is laid over config.SCENARIO_METRICS_DEFAULT_CONFIG and env.scenario_metrics() returns
    # the per-step columns, the running episode's accumulators and the last finished episode's report
    scenario_metrics=None,
)
SCENARIO_VEHICLE_CONFIG = dict(lidar=dict(num_lasers=120, distance=50), lane_line_detector=dict(num_lasers=0, distance=50),
                               side_detector=dict(num_lasers=12, distance=50))
_ONLY_SCENARIO_KEYS = ("data_directory", "start_scenario_index", "sequential_seed", "no_traffic", "no_static_vehicles", "no_light",
                       "reactive_traffic", "filter_overlapping_car", "even_sample_vehicle_class",
                       "default_vehicle_in_traffic", "on_lane_line_penalty", "crash_human_penalty",
                       "steering_range_penalty", "heading_penalty", "lateral_penalty", "max_lateral_dist",
                       "no_negative_reward", "crash_human_cost", "relax_out_of_road_done", "allowed_more_steps",
                       "walk_scenarios", "walk_stride", "scenario_pool_max_bytes", "curriculum_level",
                       "episodes_to_evaluate_curriculum", "target_success_rate", "scenario_vector_obs",
                       "traffic_lights", "skip_missing_light", "scenario_metrics")

STATIC_THRESHOLD = 3.0        # ScenarioTrafficManager.STATIC_THRESHOLD
IDM_CREATE_MIN_LENGTH = 5.0   # ScenarioTrafficManager.IDM_CREATE_MIN_LENGTH
MIN_VALID_FRAME_LEN = 20      # ScenarioTrafficManager.MIN_VALID_FRAME_LEN
ROUTE_WIDTH = 2.0             # get_idm_route(traj_points, width=2)


def make_scenario_config(user=None):
    """BaseEnv defaults + ScenarioEnv's (scenario_env.py:21-95) + the batch keys; `user` laid over them."""
    from metadrive_ped_amd.config import make_config
    user = copy.deepcopy(dict(user or {}))
    sc = copy.deepcopy(SCENARIO_DEFAULT_CONFIG)
    # agent_policy = ReplayEgoCarPolicy (policy/replay_policy.py:70-82; the reference's own scenario benchmark runs with it,
    # tests/benchmark_FPS/benchmark_waymo.py): the agent replays the SDC track, step()'s actions are ignored
    pol = user.get("agent_policy", "EnvInputPolicy")
    pol = pol if isinstance(pol, str) else getattr(pol, "__name__", repr(pol))
    ego_replay = pol == "ReplayEgoCarPolicy"
    if pol in ("ExpertPolicy", "AIProtectPolicy"):
        raise NotImplementedError("agent_policy={}: not in BatchedScenarioEnv (single-agent PG envs only)".format(pol))
    if pol == "LaneChangePolicy":
        raise NotImplementedError("agent_policy=LaneChangePolicy needs a road network's lanes: not in BatchedScenarioEnv "
                                  "(EnvInputPolicy, ReplayEgoCarPolicy)")
    if ego_replay:
        user.pop("agent_policy")
    own = {}
    for k in list(user):
        if k in _ONLY_SCENARIO_KEYS:
            own[k] = user.pop(k)
    for k in _ONLY_SCENARIO_KEYS:
        own.setdefault(k, sc[k])
    base = {k: v for k, v in sc.items() if k not in _ONLY_SCENARIO_KEYS}
    vc = copy.deepcopy(SCENARIO_VEHICLE_CONFIG)
    for k, v in (user.pop("vehicle_config", None) or {}).items():
        if isinstance(v, dict) and k in vc:
            vc[k].update(v)
        else:
            vc[k] = v
    base.update(user)
    base["vehicle_config"] = vc
    base.setdefault("traffic_density", 0.0)
    if base.get("num_pedestrians"):
        raise NotImplementedError("num_pedestrians > 0 in BatchedScenarioEnv is not built: its pedestrians come from the scenario data")
    if base.get("contact_response"):
        raise NotImplementedError("contact_response=True in BatchedScenarioEnv is not built: a scenario's replayed and trajectory-bound "
                                  "vehicles take their poses from data")
    if base.get("vector_obs") is not None:
        raise NotImplementedError("vector_obs in BatchedScenarioEnv is not built: a scenario has no lane table and its routes are "
                                  "polylines (single-agent PG envs and the multi-agent envs only)")
    cfg = make_config(base)
    cfg.update(own)
    cfg["scenario_mode"] = True
    if cfg["scenario_vector_obs"] is not None:
        from metadrive_ped_amd.config import check_scenario_vector_obs
        cfg["scenario_vector_obs"] = check_scenario_vector_obs(cfg["scenario_vector_obs"])
    if cfg["traffic_lights"] is not None:
        from metadrive_ped_amd.config import check_traffic_lights
        if cfg["no_light"]:
            raise ValueError("traffic_lights is set together with no_light=True: no_light=True asks for a batch without lights, "
                             "traffic_lights for their tables and flags; drop one of the two")
        cfg["traffic_lights"] = check_traffic_lights(cfg["traffic_lights"])
    if cfg["scenario_metrics"] is not None:
        from metadrive_ped_amd.config import check_scenario_metrics
        cfg["scenario_metrics"] = check_scenario_metrics(cfg["scenario_metrics"])
    if ego_replay:
        cfg["agent_policy"] = "ReplayEgoCarPolicy"
    if cfg["agent_policy"] == "IDMPolicy":
        raise NotImplementedError("agent_policy=IDMPolicy needs a road network: not in BatchedScenarioEnv (EnvInputPolicy, ReplayEgoCarPolicy)")
    curriculum_params(cfg)
    return cfg


def curriculum_params(cfg):
    """(n_levels, per_level, eval per worker, target) of a scenario config's curriculum, with the reference's refusals
    (envs/scenario_env.py:104-114, manager/scenario_curriculum_manager.py:41-55).  The workers are the walk's W envs.
    One level and the default window, where the reference would refuse a window that W does not divide: ceil(num_scenarios / W)."""
    L = int(cfg.get("curriculum_level", 1))
    N = int(cfg["num_scenarios"])
    W = int(cfg.get("walk_stride") or cfg["num_envs"])
    ev = cfg.get("episodes_to_evaluate_curriculum")
    if L < 1:
        raise ValueError("Curriculum Level should be greater than 1")
    if L > 1:
        if not cfg.get("walk_scenarios"):
            raise ValueError("curriculum_level > 1 needs walk_scenarios=True: without the walk an env never moves to another scenario")
        if N % L != 0:
            raise ValueError("Each level should have the same number of scenarios")
        if W > 1 and (N // L) % W != 0:
            raise ValueError("the {} scenarios per level must be divisible by num_workers (walk_stride) {}".format(N // L, W))
        if not cfg["sequential_seed"]:
            raise ValueError("Sort and sequential seed is required for curriculum seed")
    if ev is None and L == 1 and N % W != 0:
        return 1, N, -(-N // W), float(cfg.get("target_success_rate", 0.8))
    ev = int(N / L) if ev is None else int(ev)
    if ev == 0:
        raise ValueError("episodes_to_evaluate_curriculum can not be 0")
    if ev % W != 0:
        raise ValueError("Can not be divisible by num_workers")
    return L, N // L, ev // W, float(cfg.get("target_success_rate", 0.8))


def difficulty_score(sc):
    """ScenarioDataManager.sort_scenarios' _score (manager/scenario_data_manager.py:146-162): the SDC's moving distance times
    1 + the summed absolute heading changes between its consecutive valid positions over pi (the object weight is 0).  The
    distance comes from the metadata's object summary, or from the track (ScenarioDescription.sdc_moving_dist, :504-525)."""
    meta = sc["metadata"]
    sdc = meta["sdc_id"]
    st = sc["tracks"][sdc]["state"]
    xy = np.asarray(st["position"])[np.where(np.asarray(st["valid"]).astype(int))][..., :2]
    d = xy[1:] - xy[:-1]
    h = np.arctan2(d[..., 1], d[..., 0])
    curvature = sum(abs(h[1:] - h[:-1]) / np.pi) + 1
    info = (meta.get("object_summary") or {}).get(sdc) or {}
    if "moving_distance" in info:
        dist = info["moving_distance"]
    else:
        dist = float(sum(np.linalg.norm(xy[i] - xy[i + 1]) for i in range(xy.shape[0] - 1)))
    return dist * curvature


def sort_by_difficulty(scenarios):
    """(the slice in ascending difficulty, stable; the scores in that order; the original positions): the curriculum's pool"""
    scores = [difficulty_score(sc) for sc in scenarios]
    order = sorted(range(len(scenarios)), key=lambda i: scores[i])
    return [scenarios[i] for i in order], [float(scores[i]) for i in order], order


class PolyLine:
    """InterpolatingLine (utils/interpolating_line.py): consecutive points are merged until a piece is longer than 1 m;
    pieces shorter than 1e-6 are dropped; a track that never moves becomes one 0.1 m piece along +x."""
    def __init__(self, points):
        pts = np.asarray(points, dtype=np.float64)[..., :2]
        starts, ends = [], []
        i, n = 0, len(pts)
        while i < n - 1:
            j = n - 1
            for q in range(i + 1, n):
                if math.hypot(*(pts[i] - pts[q])) > 1:
                    j = q
                    break
            if math.hypot(*(pts[i] - pts[j])) >= 1e-6:
                starts.append(pts[i])
                ends.append(pts[j])
            i = j
        static = not starts
        if static:
            starts, ends = [pts[0]], [pts[0] + np.array([0.1, 0.0])]
        self.start = np.asarray(starts)
        self.end = np.asarray(ends)
        d = self.end - self.start
        self.seg_len = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)       # utils/math.py norm: sqrt(x**2 + y**2)
        self.direction = d / self.seg_len[:, None]
        self.heading = np.arctan2(d[:, 1], d[:, 0])
        self.cum = np.concatenate([[0.0], np.cumsum(self.seg_len)[:-1]])
        self.length = float(sum(self.seg_len.tolist()))           # the reference's left-to-right sum (int(length / 1.5) reads it)
        # lateral_direction = get_vertical_vector(end - start)[1] = (dy, -dx); the never-moving one-piece line has (0, 1)
        # hard-wired (interpolating_line.py:118-131) -- the device derives (dy, -dx) from the direction in every case,
        # which only differs for that degenerate line (a parked SDC: the episode ends at once, route length < 2)
        self.lateral = np.stack([self.direction[:, 1], -self.direction[:, 0]], 1)
        if static:
            self.lateral = np.array([[0.0, 1.0]])

    def _seg_at(self, s):
        """segment() / get_point(): the first piece whose accumulated end + 0.1 reaches s, else the last"""
        acc = 0.0
        for i, L in enumerate(self.seg_len):
            acc += L
            if acc + 0.1 >= s:
                return i
        return len(self.seg_len) - 1

    def position(self, s, lateral=0.0):
        i = self._seg_at(s)
        d = self.direction[i]
        return self.start[i] + (s - self.cum[i]) * d + lateral * self.lateral[i]

    def positions(self, s, lateral=0.0):
        """position() for an array of longitudinals (same piece rule: first accumulated end + 0.1 >= s, else the last)"""
        s = np.asarray(s, dtype=np.float64)
        ends = np.cumsum(self.seg_len)      # the reference accumulates in this order too
        i = np.minimum(np.searchsorted(ends + 0.1, s, side="left"), len(ends) - 1)
        return self.start[i] + (s - self.cum[i])[:, None] * self.direction[i] + lateral * self.lateral[i]

    def heading_at(self, s):
        acc = 0.0
        for i, L in enumerate(self.seg_len):
            acc += L
            if acc > s:
                return float(self.heading[i])
        return float(self.heading[-1])

    def local_coordinates(self, p):
        p = np.asarray(p, dtype=np.float64)
        sgn = ((self.start - p) * self.direction).sum(1)
        t = ((p - self.end) * self.direction).sum(1)
        h = np.maximum.reduce([sgn, t, np.zeros(len(sgn))])
        dpa = p - self.start
        c = dpa[:, 0] * self.direction[:, 1] - dpa[:, 1] * self.direction[:, 0]
        i = int(np.argmin(np.hypot(h, c)))
        d = self.direction[i]
        return float(self.cum[i] + dpa[i] @ d), float(dpa[i] @ self.lateral[i])

    def records(self):
        r = np.zeros(len(self.seg_len), dtype=abi.SEG_DT)
        r["sx"], r["sy"] = self.start[:, 0], self.start[:, 1]
        r["ex"], r["ey"] = self.end[:, 0], self.end[:, 1]
        r["dx"], r["dy"] = self.direction[:, 0], self.direction[:, 1]
        r["len"], r["heading"], r["cum"] = self.seg_len, self.heading, self.cum
        return r

    def checkpoints(self):
        """TrajectoryNavigation.discretize_reference_trajectory (trajectory_navigation.py:96-103)"""
        num = int(self.length / 2.0)
        return np.concatenate([self.positions(np.arange(num) * 2.0), self.position(self.length, 0.0)[None]])

    def outline(self, width=ROUTE_WIDTH):
        """PointLane.auto_generate_polygon (component/lane/point_lane.py:60-106): the strip of the given width sampled
        every metre, prolonged by one metre beyond both ends."""
        h0, h1 = self.heading_at(0.0), self.heading_at(self.length)
        d0 = np.array([math.cos(h0), math.sin(h0)])
        d1 = np.array([math.cos(h1), math.sin(h1)])
        longs = np.arange(0, self.length + 1.0, 1.0)
        out = []
        for side in (0, 1):
            seq = longs if side == 0 else longs[::-1]
            lat = -width / 2 if side == 0 else width / 2
            pts = self.positions(seq, lat)
            for t in range(len(seq)):
                p = pts[t]
                at_start = (t == 0 and side == 0) or (t == len(seq) - 1 and side == 1)
                at_end = (t == 0 and side == 1) or (t == len(seq) - 1 and side == 0)
                if at_start:
                    if side == 1:
                        out.append(p)
                    out.append(p - d0)
                    if side == 0:
                        out.append(p)
                elif at_end:
                    if side == 0:
                        out.append(p)
                    out.append(p + d1)
                    if side == 1:
                        out.append(p)
                else:
                    out.append(p)
        return np.asarray(out)


def _first_run(valid):
    """[t0, t1) of the first run of valid frames, or None"""
    idx = np.nonzero(valid)[0]
    if len(idx) == 0:
        return None
    t0 = int(idx[0])
    t1 = t0
    while t1 < len(valid) and valid[t1]:
        t1 += 1
    return t0, t1


def _all_runs(valid):
    """every maximal run of valid frames [t0, t1): what get_max_valid_indicis (scenario/parse_object_state.py:8-16) returns the
    end of for any frame inside it"""
    v = np.concatenate([[False], np.asarray(valid, bool), [False]])
    d = np.diff(v.astype(np.int8))
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


_KIND_OF_TYPE = {"VEHICLE": abi.KIND_VEHICLE, "PEDESTRIAN": abi.KIND_PEDESTRIAN, "CYCLIST": abi.KIND_CYCLIST,
                 "TRAFFIC_CONE": abi.KIND_CONE, "TRAFFIC_BARRIER": abi.KIND_BARRIER}


def vehicle_class_for(length, counters):
    """get_vehicle_type with even sampling (scenario_traffic_manager.py:339-361).  `counters`: the per-episode type
    counts; the reference seeds them from the traffic manager's stream, whose position depends on Bullet-side
    spawns: they start at 0 here (unpinned)."""
    if length <= 4:
        return "s"
    if length <= 5.5:
        counters[1] += 1
        return ["l", "m", "s"][counters[1] % 3]
    counters[2] += 1
    return ["l", "xl"][counters[2] % 2]


STRIPE_LENGTH = 1.5          # PGDrivableAreaProperty.STRIPE_LENGTH (constants.py:313)
_CONT_WHITE = ("UNKNOWN_LINE", "ROAD_LINE_SOLID_SINGLE_WHITE", "ROAD_LINE_SOLID_DOUBLE_WHITE",
               "UNKNOWN", "ROAD_EDGE_BOUNDARY", "ROAD_EDGE_MEDIAN")          # is_road_boundary_line -> continuous, grey
_CONT_YELLOW = ("ROAD_LINE_SOLID_SINGLE_YELLOW", "ROAD_LINE_SOLID_DOUBLE_YELLOW", "ROAD_LINE_PASSING_DOUBLE_YELLOW")
_BROKEN = ("ROAD_LINE_BROKEN_SINGLE_WHITE", "ROAD_LINE_BROKEN_SINGLE_YELLOW", "ROAD_LINE_BROKEN_DOUBLE_YELLOW")


def line_pieces(polyline, broken):
    """The stripes ScenarioBlock.construct_continuous_line / construct_broken_line cut a road line into
    (component/scenario_block/scenario_block.py:74-99): [(start, end)] in order."""
    line = PolyLine(polyline)
    if broken:
        n = int(line.length / (2 * STRIPE_LENGTH))
        k = np.arange(n, dtype=np.float64)
        sa = k * STRIPE_LENGTH * 2
        sb = k * STRIPE_LENGTH * 2 + STRIPE_LENGTH
        if n:
            sb[-1] = line.length - STRIPE_LENGTH
    else:
        n = int(line.length / STRIPE_LENGTH)
        k = np.arange(n, dtype=np.float64)
        sa = STRIPE_LENGTH * k
        sb = (k + 1) * STRIPE_LENGTH
        if n:
            sb[-1] = line.length
    if n == 0:
        return []
    pa, pb = line.positions(sa), line.positions(sb)      # get_point for all stripes at once (same piece rule)
    return [(pa[i], pb[i]) for i in range(n)]


def scene_line_quads(map_features, map_region_size):
    """Line bodies of a scenario map (ScenarioBlock.create_in_world, scenario_block.py:45-72): every road line / road
    boundary feature with at least two points, cut into stripes, each a box LANE_LINE_WIDTH / 2 wide; pieces whose
    middle lies outside the map region are not built (block/base_block.py:481).  Sidewalk / crosswalk POLYGONS are not
    turned into bodies here."""
    from metadrive_ped_amd.mapgen.tables import _line_box
    quads, kinds = [], []
    for fid, f in (map_features or {}).items():
        typ = f.get("type")
        if "polyline" not in f or len(f["polyline"]) <= 1:
            continue
        if typ in _BROKEN:
            kind, broken = abi.Q_LINE_BROKEN, True
        elif typ in _CONT_YELLOW:
            kind, broken = abi.Q_LINE_YELLOW_CONT, False
        elif typ in _CONT_WHITE:
            kind, broken = abi.Q_LINE_WHITE_CONT, False
        else:
            continue
        for a, b in line_pieces(np.asarray(f["polyline"], dtype=np.float64)[:, :2], broken):
            q = _line_box(a, b, region=map_region_size)
            if q is not None:
                quads.append(q)
                kinds.append(kind)
    return quads, kinds


# The map polylines the vector scene observation reads (include/md_scenario_vector_obs.h).  A feature's type code is its index here;
# the names are those of the reference's MetaDriveType.is_lane / is_road_line / is_road_boundary_line (type.py:109-154), in that order.
MAP_LANE_TYPES = ("LANE_SURFACE_STREET", "LANE_SURFACE_UNSTRUCTURE", "LANE_UNKNOWN", "LANE_BIKE_LANE", "LANE_FREEWAY")
MAP_LINE_TYPES = ("UNKNOWN_LINE", "ROAD_LINE_BROKEN_SINGLE_WHITE", "ROAD_LINE_SOLID_SINGLE_WHITE", "ROAD_LINE_SOLID_DOUBLE_WHITE",
                  "ROAD_LINE_BROKEN_SINGLE_YELLOW", "ROAD_LINE_BROKEN_DOUBLE_YELLOW", "ROAD_LINE_SOLID_SINGLE_YELLOW",
                  "ROAD_LINE_SOLID_DOUBLE_YELLOW", "ROAD_LINE_PASSING_DOUBLE_YELLOW")
MAP_EDGE_TYPES = ("UNKNOWN", "ROAD_EDGE_BOUNDARY", "ROAD_EDGE_MEDIAN")
MAP_FEATURE_TYPES = MAP_LANE_TYPES + MAP_LINE_TYPES + MAP_EDGE_TYPES
MAP_CLASS_LANE, MAP_CLASS_LINE, MAP_CLASS_EDGE = 0, 1, 2


def map_feature_class(type_code):
    return MAP_CLASS_LANE if type_code < len(MAP_LANE_TYPES) else \
        MAP_CLASS_LINE if type_code < len(MAP_LANE_TYPES) + len(MAP_LINE_TYPES) else MAP_CLASS_EDGE


def resample_polyline(polyline, spacing):
    """A feature's polyline at every `spacing` metres of its arc length and at its end: zero-length steps dropped, the arc length in
    float64, samples at k * spacing for k < ceil(L / spacing) and at L, linear interpolation, float32 [n, 2]; None when L < 1e-6."""
    pts = np.asarray(polyline, dtype=np.float64)[:, :2]
    step = np.hypot(*np.diff(pts, axis=0).T)
    keep = np.concatenate([[True], step > 0.0])
    pts = pts[keep]
    arc = np.concatenate([[0.0], np.cumsum(step[step > 0.0])])
    L = float(arc[-1])
    if L < 1e-6:
        return None
    at = np.concatenate([np.arange(int(math.ceil(L / spacing)), dtype=np.float64) * spacing, [L]])
    return np.stack([np.interp(at, arc, pts[:, 0]), np.interp(at, arc, pts[:, 1])], 1).astype(np.float32)


def scene_map_pieces(map_features, spacing, S):
    """The piece table of one scene: every lane / road line / road boundary feature with a polyline of at least two points, in the
    order of the dict, resampled (resample_polyline) and cut into pieces of S samples -- piece q holds samples q (S - 1) ..
    q (S - 1) + S - 1 while q (S - 1) < n - 1, so neighbours share an end point; the last one holds n_pts >= 2 samples and is padded
    with its last point.  -> (xy [pieces, S, 2] float32, info [pieces, 4] int32: class, type code, n_pts, the feature's ordinal among
    the dict's features).  Polygons (crosswalks, sidewalks, speed bumps), stop signs and driveways are skipped."""
    xy, info = [], []
    for ordinal, f in enumerate((map_features or {}).values()):
        typ = f.get("type")
        if typ not in MAP_FEATURE_TYPES or "polyline" not in f or len(f["polyline"]) < 2:
            continue
        pts = resample_polyline(f["polyline"], spacing)
        if pts is None:
            continue
        code, n = MAP_FEATURE_TYPES.index(typ), len(pts)
        q = 0
        while q * (S - 1) < n - 1:
            piece = pts[q * (S - 1):q * (S - 1) + S]
            n_pts = len(piece)
            xy.append(np.concatenate([piece, np.repeat(piece[-1:], S - n_pts, axis=0)]))
            info.append((map_feature_class(code), code, n_pts, ordinal))
            q += 1
    return (np.asarray(xy, np.float32).reshape(-1, S, 2), np.asarray(info, np.int32).reshape(-1, 4))


def map_piece_balls(xy, info):
    """[pieces, 4] float32: a circle around every piece's n_pts points, as _poly_balls makes them -- the centre the middle of the
    points' bounding box, the radius the farthest point in float64, stored as float32 with the radius rounded UP past the centre's
    rounding and a 1e-3 m margin -- the kernel's exact cull."""
    out = np.zeros((len(xy), 4), np.float32)
    if len(xy) == 0:
        return out
    p = xy.astype(np.float64)                   # a padded point repeats the last one: it changes neither the box nor the radius
    cx = (0.5 * (p[:, :, 0].min(1) + p[:, :, 0].max(1))).astype(np.float32)
    cy = (0.5 * (p[:, :, 1].min(1) + p[:, :, 1].max(1))).astype(np.float32)
    r = np.hypot(p[:, :, 0] - cx.astype(np.float64)[:, None], p[:, :, 1] - cy.astype(np.float64)[:, None]).max(1)
    out[:, 0], out[:, 1] = cx, cy
    out[:, 2] = np.nextafter((r + 1.0e-3 + 1.0e-6 * (np.abs(cx) + np.abs(cy))).astype(np.float32), np.float32(np.inf))
    return out


def map_piece_tables(per_scene, S, max_scene_pieces=None):
    """The tables of MdScenarioVectorObs over the scenes' (xy, info) pairs: dict(map_off [scenes + 1], map_xy, map_info, map_ball,
    max_pieces).  A scene with more pieces than MD_SVO_MAX_PIECES is refused."""
    limit = abi.MD_SVO_MAX_PIECES if max_scene_pieces is None else max_scene_pieces
    counts = [len(xy) for xy, _ in per_scene]
    for q, n in enumerate(counts):
        if n > limit:
            raise ValueError("scenario_vector_obs: scene {} has {} map polyline pieces, more than MD_SVO_MAX_PIECES={}: raise "
                             "map_spacing or piece_points".format(q, n, limit))
    xy = np.concatenate([xy for xy, _ in per_scene]) if sum(counts) else np.zeros((0, S, 2), np.float32)
    info = np.concatenate([i for _, i in per_scene]) if sum(counts) else np.zeros((0, 4), np.int32)
    pad = 1 if len(xy) == 0 else 0               # never an empty device array
    return dict(map_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                map_xy=np.concatenate([xy, np.zeros((pad, S, 2), np.float32)]), map_info=np.concatenate([info, np.zeros((pad, 4), np.int32)]),
                map_ball=np.concatenate([map_piece_balls(xy, info), np.zeros((pad, 4), np.float32)]), max_pieces=int(max(counts + [0])))


# The traffic lights of a description's dynamic_map_states (include/md_traffic_lights.h): ScenarioLightManager._get_episode_light_data /
# after_reset (manager/scenario_light_manager.py:31-52,83-106) and BaseTrafficLight.__init__ (component/traffic_light/
# base_traffic_light.py:44-60), restated once per scene.
AIR_WALL_LENGTH = 0.25        # BaseTrafficLight.AIR_WALL_LENGTH: the wall's extent ALONG the lane
LIGHT_LANE_WIDTH = 6.0        # ScenarioLane.VIS_LANE_WIDTH (component/lane/scenario_lane.py:23,43): width_at(0) of every scenario lane
PLACE_LONGITUDE = 5.0         # BaseTrafficLight.PLACE_LONGITUDE: the wall's heading is the lane's at 5 m, wherever the wall stands
_LIGHT_CODES = dict(
    LANE_STATE_ARROW_STOP=abi.TL_RED, LANE_STATE_STOP=abi.TL_RED, TRAFFIC_LIGHT_RED=abi.TL_RED,
    LANE_STATE_ARROW_CAUTION=abi.TL_YELLOW, LANE_STATE_CAUTION=abi.TL_YELLOW, LANE_STATE_FLASHING_CAUTION=abi.TL_YELLOW,
    TRAFFIC_LIGHT_YELLOW=abi.TL_YELLOW,
    LANE_STATE_ARROW_GO=abi.TL_GREEN, LANE_STATE_GO=abi.TL_GREEN, TRAFFIC_LIGHT_GREEN=abi.TL_GREEN)


def light_status_code(status):
    """MetaDriveType.simplify_light_status (type.py:221-236) as a code: 0 unknown (None, LANE_STATE_UNKNOWN, LANE_STATE_FLASHING_STOP,
    TRAFFIC_LIGHT_UNKNOWN and any string it does not list), 1 green, 2 yellow, 3 red"""
    if status is None:
        return abi.TL_UNKNOWN
    if isinstance(status, bytes):
        status = status.decode()
    return _LIGHT_CODES.get(str(status), abi.TL_UNKNOWN)


def _light_position(entry):
    """_get_episode_light_data's position (scenario_light_manager.py:89-103): the old format keeps a [T, 2] array under
    state["stop_point"] and takes the row of the first frame whose state["lane"] is not 0 (the last row, first_pos = -1, when there
    is none); the new format keeps one point at the entry's top level"""
    state = entry["state"]
    if "stop_point" in state:
        rows = np.asarray(state["stop_point"], np.float64)
        lane = np.asarray(state["lane"])
        lane = lane.astype(np.float64) if lane.dtype.kind in "biuf" else np.asarray([float(x or 0) for x in lane.ravel()])
        on = np.nonzero(lane != 0)[0]
        return rows[int(on[0]) if len(on) else -1][:2]
    return np.asarray(entry["stop_point"], np.float64)[:2]


def scene_traffic_lights(scenario, skip_missing_light=True):
    """The lights of one scenario description -> (box [n, 8] float32, status: a list of n uint8 arrays, ids: the n kept keys of
    dynamic_map_states).  One light per key, in the dict's order -- its position among the kept keys is the light's ordinal.  The
    lane is the map feature str(key), which must be a lane (a type of MAP_LANE_TYPES: the reference looks the key up among the road
    network's lanes); a light without one is skipped, or refused with skip_missing_light=False.  The wall: centred on the position,
    AIR_WALL_LENGTH along and the lane's 6 m across the heading the lane has at PLACE_LONGITUDE -- generate_static_box_physics_body
    (utils/pg/utils.py:315) makes BulletBoxShape(heading_length / 2, side_width / 2, ...), so the SHORT side lies along the heading."""
    feats = scenario.get("map_features") or {}
    box, status, ids = [], [], []
    for key, entry in (scenario.get("dynamic_map_states") or {}).items():
        if entry.get("type") != "TRAFFIC_LIGHT":
            raise ValueError("Can not handle {}".format(entry.get("type")))        # the reference's assert, with its message
        pos = _light_position(entry)
        lane = feats.get(str(key))
        if lane is None or lane.get("type") not in MAP_LANE_TYPES or "polyline" not in lane or len(lane["polyline"]) < 2:
            if skip_missing_light:
                continue
            raise ValueError("Can not find lane for this traffic light. Set skip_missing_light=True for skipping missing light!")
        heading = PolyLine(lane["polyline"]).heading_at(PLACE_LONGITUDE)
        box.append((pos[0], pos[1], math.cos(heading), math.sin(heading), 0.5 * AIR_WALL_LENGTH, 0.5 * LIGHT_LANE_WIDTH, 0.0, 0.0))
        codes = [light_status_code(x) for x in np.asarray(entry["state"]["object_state"], dtype=object).ravel()]
        status.append(np.asarray(codes or [abi.TL_UNKNOWN], np.uint8))              # never an empty array: one unknown frame
        ids.append(key)
    return np.asarray(box, np.float32).reshape(-1, 8), status, ids


def traffic_light_tables(per_scene, max_scene_lights=None):
    """The tables of MdTrafficLights over the scenes' (box, status, ids) triples: dict(tl_off [scenes + 1], tl_box [lights, 8],
    tl_info [lights, 4] (status offset, frames, ordinal, 0), tl_status, max_scene_lights, ids: the kept keys per scene).  A scene
    with more lights than MD_TL_MAX_SCENE_LIGHTS is refused; one without lights is legal."""
    limit = abi.MD_TL_MAX_SCENE_LIGHTS if max_scene_lights is None else max_scene_lights
    counts = [len(box) for box, _, _ in per_scene]
    for q, n in enumerate(counts):
        if n > limit:
            raise ValueError("traffic_lights: scene {} has {} traffic lights, more than MD_TL_MAX_SCENE_LIGHTS={}".format(q, n, limit))
    box = np.concatenate([b for b, _, _ in per_scene]) if sum(counts) else np.zeros((0, 8), np.float32)
    info, status, at = [], [], 0
    for _, st, _ in per_scene:
        for ordinal, codes in enumerate(st):
            info.append((at, len(codes), ordinal, 0))
            status.append(codes)
            at += len(codes)
    pad = 1 if len(box) == 0 else 0               # never an empty device array
    return dict(tl_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                tl_box=np.concatenate([box, np.zeros((pad, 8), np.float32)]),
                tl_info=np.concatenate([np.asarray(info, np.int32).reshape(-1, 4), np.zeros((pad, 4), np.int32)]),
                tl_status=np.concatenate(status + [np.zeros(1, np.uint8)]),       # one spare byte: never empty
                max_scene_lights=int(max(counts + [0])), ids=[list(ids) for _, _, ids in per_scene])


def _to_frames(a, T):
    """first T frames of a per-frame array, zero / False padded"""
    a = np.asarray(a)
    if len(a) >= T:
        return a[:T]
    out = np.zeros((T, ) + a.shape[1:], dtype=a.dtype)
    out[:len(a)] = a
    return out


def _build_scene(job):
    """One scenario description -> the per-scene arrays (module-level so that a fork pool can run it)."""
    from metadrive_ped_amd.scene import vehicle_param_record
    from metadrive_ped_amd.rng import get_np_random
    e, sc, cap, T, seed, dt, no_traffic, region, svo, tl = job
    shape0 = np.zeros(cap, dtype=abi.SHAPE_DT)
    shape0["aux"] = -1
    dyn0 = np.zeros(cap, dtype=abi.DYN_DT)
    param = np.zeros(cap, dtype=abi.PARAM_DT)
    param["max_speed_kmh"], param["lf"], param["lr"] = 80.0, 1.0, 1.0
    fshape = np.zeros((T, cap), dtype=abi.SHAPE_DT)
    fshape["aux"] = -1
    fdyn = np.zeros((T, cap, 2), np.float32)
    meta = np.zeros((cap, 4), np.int32)
    meta[:, 2] = abi.TM_NEVER
    runs = [[] for _ in range(cap)]      # vehicles: all valid runs (a route cut at a later spawn frame ends with its run)
    cut_frames, cut_metres = 1, 1.0      # bounds of such a route: frames of the longest run, its path length
    sdc_id = str(sc["metadata"]["sdc_id"])
    order = [sdc_id] + [str(k) for k in sc["tracks"] if str(k) != sdc_id]
    counters = [0, 0, 0]
    polys = [None] * cap
    ck = None
    for j, oid in enumerate(order):
        tr = sc["tracks"][oid] if oid in sc["tracks"] else sc["tracks"][int(oid)]
        st = tr["state"]
        valid = np.asarray(st["valid"]).astype(bool)
        pos = np.asarray(st["position"], dtype=np.float64)[:, :2]
        heading = np.asarray(st["heading"], dtype=np.float64)
        vel = np.asarray(st["velocity"], dtype=np.float64)
        own_len = len(pos)
        if own_len != T:   # a batch of scenes of different lengths: shorter ones end with invalid frames
            valid, pos, heading, vel = (_to_frames(a, T) for a in (valid, pos, heading, vel))
        n = j
        run = _first_run(valid)
        if j == 0:
            # the agent: default vehicle at the SDC's first frame (scenario_map_manager.py:55-75); its route =
            # the whole track up to the first > 100 m jump (parse_full_trajectory, parse_object_state.py:77-90)
            cut = own_len
            for t in range(own_len - 1):
                if math.hypot(*(pos[t] - pos[t + 1])) > 100:
                    cut = t
                    break
            polys[0] = PolyLine(pos[:cut])
            prm, length, width, _ = vehicle_param_record("default", int(get_np_random(seed).randint(0, 2 ** 16)), dt)
            param[n] = prm
            h = float(heading[0])
            sh = shape0[n]
            sh["cx"], sh["cy"], sh["c"], sh["s"] = pos[0, 0], pos[0, 1], math.cos(h), math.sin(h)
            sh["hl"], sh["hw"] = length / 2, width / 2
            sh["flags"] = abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT
            shape0[n] = sh
            d = dyn0[n]
            d["heading"], d["speed"] = h, float(vel[0, 0] * math.cos(h) + vel[0, 1] * math.sin(h))
            d["last_x"], d["last_y"], d["last_c"], d["last_s"] = pos[0, 0], pos[0, 1], math.cos(h), math.sin(h)
            dyn0[n] = d
            meta[n] = (0, int(sc.get("length", own_len)), abi.TM_NEVER, 0)   # [1] = this scene's current_scenario_length
            ck = polys[0].checkpoints()
            # the SDC's own frames (read only with agent_policy = ReplayEgoCarPolicy)
            f = fshape[:, 0]
            f["cx"][valid], f["cy"][valid] = pos[valid, 0], pos[valid, 1]
            f["c"][valid], f["s"][valid] = np.cos(heading[valid]), np.sin(heading[valid])
            f["hl"][valid], f["hw"][valid] = length / 2, width / 2
            f["flags"][valid] = abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT
            fshape[:, 0] = f
            fdyn[valid, 0, 0] = heading[valid]
            fdyn[valid, 0, 1] = np.hypot(vel[valid, 0], vel[valid, 1])
            continue
        kind = _KIND_OF_TYPE.get(tr["type"])
        if kind is None or run is None or no_traffic:
            continue
        t0, t1 = run
        flags = 0
        if kind == abi.KIND_VEHICLE:
            vp = pos[valid]
            if float(np.max(np.std(vp, axis=0)[:2])) > STATIC_THRESHOLD:
                flags |= abi.TM_MOVING
            if math.hypot(*(pos[t0] - pos[t1 - 1])) > IDM_CREATE_MIN_LENGTH:
                flags |= abi.TM_LENGTH_OK
            rec_len = float(np.asarray(st["length"])[t0]) if "length" in st else 4.5
            vtype = vehicle_class_for(rec_len, counters)
            prm, length, width, _ = vehicle_param_record(vtype, int(get_np_random(seed * 131 + j).randint(0, 2 ** 16)), dt)
            param[n] = prm
            hl, hw = length / 2, width / 2
            polys[j] = PolyLine(pos[t0:t1])
            runs[j] = _all_runs(valid)
            for a_, b_ in runs[j]:
                cut_frames = max(cut_frames, b_ - a_)
                if b_ - a_ > 1:
                    step = np.diff(pos[a_:b_], axis=0)
                    cut_metres = max(cut_metres, float(np.sqrt((step ** 2).sum(1)).sum()))
        elif kind == abi.KIND_PEDESTRIAN:
            hl = hw = 0.35
        elif kind == abi.KIND_CYCLIST:
            hl, hw = 0.875, 0.2
        elif kind == abi.KIND_CONE:
            hl = hw = 0.2
            if int(valid.sum()) < MIN_VALID_FRAME_LEN:
                flags |= abi.TM_NEVER
        else:
            hl, hw = 0.15, 1.0
            if int(valid.sum()) < MIN_VALID_FRAME_LEN:
                flags |= abi.TM_NEVER
        meta[n] = (t0, t1, flags, 0)
        f = fshape[:, n]
        f["cx"][valid], f["cy"][valid] = pos[valid, 0], pos[valid, 1]
        f["c"][valid], f["s"][valid] = np.cos(heading[valid]), np.sin(heading[valid])
        f["hl"][valid], f["hw"][valid] = hl, hw
        fl = kind | abi.F_ALIVE
        if kind in (abi.KIND_CONE, abi.KIND_BARRIER):
            fl |= abi.F_STATIC
        f["flags"][valid] = fl
        fshape[:, n] = f
        fdyn[valid, n, 0] = heading[valid]
        fdyn[valid, n, 1] = np.hypot(vel[valid, 0], vel[valid, 1])
        # a free slot still carries the class's size, so that the device only rewrites the pose on a spawn
        shape0[n]["hl"], shape0[n]["hw"] = hl, hw
    segs, verts = [], []
    for j in range(cap):
        pl = polys[j]
        segs.append(pl.records() if pl is not None else np.zeros(0, dtype=abi.SEG_DT))
        want_outline = j > 0 and pl is not None and (meta[j, 2] & abi.TM_MOVING) and (meta[j, 2] & abi.TM_LENGTH_OK)
        verts.append(pl.outline() if want_outline else np.zeros((0, 2)))
    from metadrive_ped_amd.mapgen.tables import StaticTables
    static = StaticTables(*scene_line_quads(sc.get("map_features"), region))      # road-line bodies + their grid
    # the vector scene observation's piece table (svo: None, or its (map_spacing, piece_points))
    map_pieces = scene_map_pieces(sc.get("map_features"), *svo) if svo is not None else None
    # the traffic lights' walls and statuses (tl: None, or skip_missing_light)
    lights = scene_traffic_lights(sc, tl) if tl is not None else None
    return dict(shape0=shape0, dyn0=dyn0, param=param, fshape=fshape, fdyn=fdyn, meta=meta, order=order, segs=segs, verts=verts, ckpt=ck,
                static=static, runs=runs, cut_frames=cut_frames, cut_metres=cut_metres, map_pieces=map_pieces,
                lights=lights)



def walk_params(cfg):
    """(n_scenes, mode, W, offset, seed) of MdState.walk for a scenario config: mode 0 off, 1 sequential, 2 uniform"""
    if not cfg.get("walk_scenarios"):
        return 0, 0, 0, 0, 0
    W = int(cfg.get("walk_stride") or cfg["num_envs"])
    return (int(cfg["num_scenarios"]), 1 if cfg["sequential_seed"] else 2, W, int(cfg.get("env_seed_offset", 0)),
            int(cfg.get("start_seed", 0)) & 0xFFFFFFFF)


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def walk_scene(cfg, e, ep):
    """The scene (index into the slice [start_scenario_index, + num_scenarios)) env e plays in episode ep of its walk
    (0 = the first after a reset): md_walk_scene of include/md_scenario.h, restated for arrays of e / ep.
    sequential_seed: ScenarioEnv._reset_global_seed (envs/scenario_env.py:359-380) with env e as worker
    w = (env_seed_offset + e) % num_scenarios of W = walk_stride workers -- w, w + W, w + 2W, ... while inside the slice, then w
    again; otherwise a draw over the slice keyed by (start_seed, env_seed_offset + e, ep)."""
    n, walk, W, off, seed = walk_params(cfg)
    e = np.asarray(e, np.int64)
    ep = np.asarray(ep, np.int64)
    if walk == 2:
        with np.errstate(over="ignore"):
            key = (np.uint64(seed) << np.uint64(32)) | ((off + e) & 0xFFFFFFFF).astype(np.uint64)
            z = _mix(_mix(key) ^ ((ep & 0xFFFFFFFF).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)))
            return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    w = (off + e) % n
    m = (n - w + W - 1) // W
    return w + (ep % m) * W


class _World:
    def __init__(self, arrays, n_envs):
        self.arrays = arrays
        self.n_maps = 1
        self.n_envs = n_envs


def _poly_aux(poly_off, segs, polyv_off, polyv):
    """MdWorld.poly_aux: per slot the polyline's end point -- float32 arithmetic in the order of md_poly_position(p, length, 0):
    the first piece with cum + len + 0.1 >= length, then sx + (length - cum) * dx -- and the bounding box of the outline."""
    f = np.float32
    n_slot = len(poly_off) - 1
    out = np.zeros((n_slot, 8), np.float32)
    for k in range(n_slot):
        a, b = int(poly_off[k]), int(poly_off[k + 1])
        if b > a:
            g = segs[a:b]
            length = f(g["cum"][-1]) + f(g["len"][-1])
            ends = (g["cum"].astype(f) + g["len"].astype(f)) + f(0.1)
            hit = np.nonzero(ends >= length)[0]
            ge = g[int(hit[0]) if len(hit) else b - a - 1]
            along = length - f(ge["cum"])
            out[k, 0] = f(ge["sx"]) + along * f(ge["dx"])
            out[k, 1] = f(ge["sy"]) + along * f(ge["dy"])
        va, vb = int(polyv_off[k]), int(polyv_off[k + 1])
        if vb > va:
            v = polyv[va:vb]
            out[k, 2:6] = v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()
        else:
            out[k, 2:6] = 1.0, 1.0, -1.0, -1.0      # empty box: nothing is inside
    return out


def _poly_balls(poly_off, segs):
    """MdWorld.poly_ball / poly_ball_off: a circle around every group of MD_POLY_GROUP consecutive pieces of a slot's polyline
    (centre = middle of the end points' bounding box, radius = farthest end point, in float64; stored as float32 with the radius
    rounded UP past the centre's rounding and a 1e-3 m margin): the projections' exact cull."""
    G = abi.MD_POLY_GROUP
    po = np.asarray(poly_off, np.int64)
    n_g = (np.diff(po) + G - 1) // G
    off = np.zeros(len(po), np.int64)
    off[1:] = np.cumsum(n_g)
    total = int(off[-1])
    out = np.zeros((max(total, 1), 4), np.float32)
    if total == 0:
        return out, off.astype(np.int32)
    # first piece of every group, in order (the pieces of a group are contiguous in `segs`)
    starts = np.repeat(po[:-1], n_g) + G * (np.arange(total) - np.repeat(off[:-1], n_g))
    count = np.minimum(G, np.repeat(po[1:], n_g) - starts)
    gid = np.repeat(np.arange(total), count)             # group of every piece of every polyline (pieces outside polylines: none)
    piece = np.repeat(starts, count) + (np.arange(len(gid)) - np.repeat(np.cumsum(count) - count, count))
    sx, sy = segs["sx"][piece].astype(np.float64), segs["sy"][piece].astype(np.float64)
    ex, ey = segs["ex"][piece].astype(np.float64), segs["ey"][piece].astype(np.float64)
    first = np.cumsum(count) - count
    xmin = np.minimum(np.minimum.reduceat(sx, first), np.minimum.reduceat(ex, first))
    xmax = np.maximum(np.maximum.reduceat(sx, first), np.maximum.reduceat(ex, first))
    ymin = np.minimum(np.minimum.reduceat(sy, first), np.minimum.reduceat(ey, first))
    ymax = np.maximum(np.maximum.reduceat(sy, first), np.maximum.reduceat(ey, first))
    cx, cy = (0.5 * (xmin + xmax)).astype(np.float32), (0.5 * (ymin + ymax)).astype(np.float32)
    cxd, cyd = cx.astype(np.float64)[gid], cy.astype(np.float64)[gid]
    d = np.maximum(np.hypot(sx - cxd, sy - cyd), np.hypot(ex - cxd, ey - cyd))
    r = np.maximum.reduceat(d, first)
    out[:total, 0], out[:total, 1] = cx, cy
    out[:total, 2] = np.nextafter((r + 1.0e-3 + 1.0e-6 * (np.abs(cx) + np.abs(cy))).astype(np.float32), np.float32(np.inf))
    return out, off.astype(np.int32)


def curriculum_state(E, n_scenes, eval_):
    """The curriculum's per-env arrays (include/md_curriculum.h MdCurriculum, keys cur_*) of a batch before its first reset:
    every env at level 0, no seed yet, empty queues of `eval_` entries, nothing of the `n_scenes` scenes covered."""
    return dict(cur_level=np.zeros(E, np.int32), cur_seed=np.full(E, -1, np.int32), cur_q_len=np.zeros(E, np.int32),
                cur_q_key=np.full((E, eval_), -1, np.int32), cur_q_success=np.zeros((E, eval_), np.int32),
                cur_q_route=np.zeros((E, eval_), np.float32), cur_cover=np.zeros((E, (n_scenes + 31) // 32), np.uint32),
                cur_cover_n=np.zeros(E, np.int32), cur_rep_i=np.zeros((E, 2), np.int32), cur_rep_f=np.zeros((E, 3), np.float64))


class ScenarioHostScene(HostSceneBase):
    """The HostScene of scenario mode: one scenario description per env (`scenarios[e]` -> env e), or -- with walk_scenarios --
    the scene pool of the dataset slice (`scenarios[p]` = scenario start_scenario_index + p), every scene built once, that the
    envs walk through (walk_scene; the device moves an env on in md_swap_draw)."""
    def __init__(self, cfg, scenarios):
        self.cfg = cfg
        self.E, self.A, self.walk = cfg["num_envs"], 1, bool(cfg.get("walk_scenarios"))
        self.spawn, self.traffic_respawns, self.scenes = None, False, {}
        ObsLayout(cfg, scenario=True).export_to(self)      # self.layout, and n_beams / n_side / n_ll / ... / obs_dim
        scenarios, order = self._assign_scenes(scenarios)
        self._sizes(scenarios)
        built = self._build(scenarios, order)
        self._world_tables(built)
        self._state(built)
        self._md_config()
        if self.walk:
            dev_bytes = sum(v.nbytes for d in (self.world.arrays, self.pool) for v in d.values()) + self.tracks["shape"].nbytes \
                + self.tracks["dyn"].nbytes
            print("walk_scenarios: scene pool of num_scenarios={} scenes (T={}, mover capacity {}): {:.1f} MiB on the device".format(
                len(scenarios), self.T, self.cap, dev_bytes / 2 ** 20))
        self.set_detector_beams()

    def _assign_scenes(self, scenarios):
        """-> (the scenarios in pool order, their order in the slice or None); sets env_scene (the scene of every env: its own, or
        the first of its walk), curriculum and difficulty."""
        cfg, E = self.cfg, self.E
        self.curriculum, self.difficulty = None, None
        if not self.walk:
            if len(scenarios) != E:
                raise ValueError("need one scenario per env: got {} for {} envs".format(len(scenarios), E))
            self.env_scene = list(range(E))
            return scenarios, None
        P = int(cfg["num_scenarios"])
        if len(scenarios) != P:
            raise ValueError("walk_scenarios: need the num_scenarios={} scenarios of the slice, got {}".format(P, len(scenarios)))
        self.env_scene = [int(p) for p in walk_scene(cfg, np.arange(E), 0)]     # every env at the first scene of its walk
        # the curriculum: the slice sorted by difficulty before the pool is built (ScenarioDataManager.sort_scenarios runs
        # with more than one level only; scenario_difficulty is 0 otherwise)
        self.curriculum = curriculum_params(cfg)
        if self.curriculum[0] > 1:
            scenarios, diff, order = sort_by_difficulty(scenarios)
            self.difficulty = np.asarray(diff, np.float64)
            return scenarios, order
        self.difficulty = np.zeros(P, np.float64)
        return scenarios, None

    def _sizes(self, scenarios):
        """T, cap and the identity of the scenes (seeds, scenario_ids)"""
        cfg, S = self.cfg, len(scenarios)
        T = max(int(sc["length"]) for sc in scenarios)   # frames of the batch; a shorter scene is over (all invalid) after its own
        n_tracks = max(len(sc["tracks"]) for sc in scenarios)
        cap = cfg["mover_capacity"] or min(abi.MD_MAX_CAP, max(8, (n_tracks + 7) // 8 * 8))
        if n_tracks > cap:
            raise ValueError("a scenario holds {} objects, the mover capacity is {}".format(n_tracks, cap))
        if self.walk:
            # the recorded frames dominate the pool: T x scenes x cap x (MdShape + heading, speed)
            frames = T * S * cap * (abi.SHAPE_DT.itemsize + 8)
            if frames > int(cfg["scenario_pool_max_bytes"]):
                raise ValueError("walk_scenarios: the pool of num_scenarios={} scenes needs {:.2f} GiB of recorded frames alone "
                                 "(T={}, mover capacity {}), more than scenario_pool_max_bytes={:.2f} GiB: walk a smaller slice".format(
                                     S, frames / 2 ** 30, T, cap, int(cfg["scenario_pool_max_bytes"]) / 2 ** 30))
        self.cap, self.T = cap, T
        # scene e <-> dataset index start_scenario_index + (env_seed_offset + e) % num_scenarios (scenario_data.scenario_indices):
        # the identity checkpoints and track sets are checked against, and the fallback parameter seed of a description that
        # carries none -- tied to WHICH scenario it is, not to where it sits in the batch.  A walk's pool: the slice itself.
        from metadrive_ped_amd.scenario_data import scenario_indices
        self.seeds = [int(cfg["start_scenario_index"]) + p for p in range(S)] if self.walk else scenario_indices(cfg, self.E)
        self.scenario_ids = [str(sc.get("id", sc.get("metadata", {}).get("scenario_id", i))) for sc, i in zip(scenarios, self.seeds)]

    def _build(self, scenarios, order):
        """Every scene once, through the build workers.  Vehicle parameters are sampled from a stream seeded by the scenario's OWN
        seed where it carries one, so that a scene behaves the same in whatever batch (slot, shard) it is loaded."""
        from metadrive_ped_amd import hostpool
        cfg = self.cfg
        fallback = self.seeds if order is None else [int(cfg["start_scenario_index"]) + i for i in order]   # the dataset index
        vo = cfg.get("scenario_vector_obs")
        svo = (float(vo["map_spacing"]), int(vo["piece_points"])) if vo is not None and int(vo["num_pieces"]) > 0 else None
        tl = bool(cfg.get("skip_missing_light", True)) if cfg.get("traffic_lights") is not None else None
        jobs = [(p, sc, self.cap, self.T, int(sc["metadata"].get("seed", fallback[p])), cfg["physics_world_step_size"],
                 bool(cfg["no_traffic"]), float(cfg["map_region_size"]), svo, tl) for p, sc in enumerate(scenarios)]
        built = hostpool.build_all(_build_scene, jobs, workers=int(cfg.get("build_workers", 0)))
        self.track_ids = [b_["order"] for b_ in built]
        # the vector scene observation's map polyline pieces, per scene (None without the key, or with num_pieces 0)
        self.map_pieces = map_piece_tables([b_["map_pieces"] for b_ in built], svo[1]) if svo is not None else None
        # the traffic lights' tables, per scene, and the kept keys of dynamic_map_states in ordinal order (None without the key)
        self.traffic_lights = traffic_light_tables([b_["lights"] for b_ in built]) if tl is not None else None
        self.traffic_light_ids = self.traffic_lights["ids"] if tl is not None else None
        self.tracks = dict(shape=np.concatenate([b_["fshape"] for b_ in built], axis=1),
                           dyn=np.concatenate([b_["fdyn"] for b_ in built], axis=1), seeds=list(self.seeds), cap=self.cap)
        return built

    def _world_tables(self, built):
        """Static bodies: one map per scene (its road lines + their grid); the lane / road / node tables are placeholders.  On
        top of them the scenes' polylines, outlines, checkpoints, track records and runs, each with its offset table."""
        from metadrive_ped_amd.mapgen.tables import WorldTables
        segs, poly_off, verts, polyv_off, ckpts, ckpt_off = [], [0], [], [0], [], [0]
        for b_ in built:
            for r in b_["segs"]:
                segs.append(r)
                poly_off.append(poly_off[-1] + len(r))
            for v in b_["verts"]:
                verts.append(v)
                polyv_off.append(polyv_off[-1] + len(v))
            ckpts.append(b_["ckpt"])
            ckpt_off.append(ckpt_off[-1] + len(b_["ckpt"]))
        self.map_tables = [b_["static"] for b_ in built]
        self.world = WorldTables(self.map_tables, list(self.env_scene), beam_table(self.n_beams))
        a = self.world.arrays
        a["poly_off"] = np.asarray(poly_off, np.int32)
        a["segs"] = np.concatenate(segs) if sum(len(x) for x in segs) else np.zeros(1, dtype=abi.SEG_DT)
        a["polyv_off"] = np.asarray(polyv_off, np.int32)
        vv = np.concatenate(verts) if sum(len(x) for x in verts) else np.zeros((1, 2))
        a["polyv"] = np.ascontiguousarray(vv, dtype=np.float32)
        a["ckpt_off"] = np.asarray(ckpt_off, np.int32)
        a["ckpt_xy"] = np.ascontiguousarray(np.concatenate(ckpts), dtype=np.float32)
        a["track_meta"] = np.concatenate([b_["meta"] for b_ in built])
        run_off, run_list = [0], []
        for b_ in built:
            for r in b_["runs"]:
                run_list.extend(r)
                run_off.append(run_off[-1] + len(r))
        a["run_off"] = np.asarray(run_off, np.int32)
        a["runs"] = np.asarray(run_list if run_list else [(0, 0)], np.int32).reshape(-1, 2)
        a["poly_aux"] = _poly_aux(a["poly_off"], a["segs"], a["polyv_off"], a["polyv"])
        a["poly_ball"], a["poly_ball_off"] = _poly_balls(a["poly_off"], a["segs"])
        # buffers for routes cut at a later spawn frame (MdState.route_*): at most one piece per frame of the longest run, the
        # outline two vertices per metre of its path + the end caps
        self.route_seg_cap = int(max(b_["cut_frames"] for b_ in built))
        self.route_vert_cap = 2 * (int(math.ceil(max(b_["cut_metres"] for b_ in built))) + 3) + 4

    def _state(self, built):
        cfg, E, cap, S = self.cfg, self.E, self.cap, len(built)
        N = E * cap
        nav0 = np.zeros(N, dtype=abi.NAV_DT)
        nav0["lane"], nav0["target_lane"], nav0["road0"], nav0["road1"] = -1, -1, -1, -1
        pid0 = np.zeros(N, dtype=abi.PID_DT)
        pid0["target_speed"] = 40.0
        rows = {k: np.concatenate([built[p][k] for p in self.env_scene]) for k in ("shape0", "dyn0", "param")}
        rows.update(nav0=nav0, pid0=pid0, route_nodes=np.full((N, abi.MD_ROUTE_LEN), -1, np.int32),
                    route_roads=np.full((N, abi.MD_ROUTE_LEN), -1, np.int32), final_lane=np.zeros(N, np.int32),
                    idm_rand=np.zeros((N, abi.MD_IDM_RAND), np.int32))
        st = step_state(E, self.A, cap, self.obs_dim, rows, self.env_scene if self.walk else None)
        st["next_agent_id"] = np.zeros(E, np.int32)     # ScenarioTrafficManager.idm_policy_count
        self.pool = None
        if self.walk:   # the snapshot rows of every scene, at p * cap: what md_swap_draw copies into an env that moves on to scene p
            self.pool = {k: np.concatenate([b_[k] for b_ in built]) for k in ("shape0", "dyn0", "param")}
            self.pool.update(nav0=np.resize(nav0[:cap], S * cap), pid0=np.resize(pid0[:cap], S * cap))
            st.update(curriculum_state(E, S, self.curriculum[2]))
        if cfg["reactive_traffic"]:
            st["route_n"] = np.zeros((N, 4), np.int32)
            st["route_segs"] = np.zeros((N, self.route_seg_cap), dtype=abi.SEG_DT)
            st["route_verts"] = np.zeros((N, self.route_vert_cap, 2), np.float32)
            st["route_aux"] = np.zeros((N, 8), np.float32)
        self.state = st

    def _md_config(self):
        from metadrive_ped_amd.engine import make_md_config
        cfg = self.cfg
        k = make_md_config(dict(cfg, traffic_mode="trigger"), self.layout, self.E, self.A, self.cap)
        k.traffic_mode = 4
        k.track_len = k.scenario_length = self.T
        for name in ("on_lane_line_penalty", "crash_human_penalty", "steering_range_penalty", "heading_penalty",
                     "lateral_penalty", "max_lateral_dist", "crash_human_cost"):
            setattr(k, name, float(cfg[name]))
        for name in ("no_negative_reward", "relax_out_of_road_done", "reactive_traffic", "filter_overlapping_car",
                     "no_static_vehicles"):
            setattr(k, name, int(bool(cfg[name])))
        k.allowed_more_steps = int(cfg["allowed_more_steps"] or 0)
        k.route_seg_cap, k.route_vert_cap = self.route_seg_cap, self.route_vert_cap
        k.ego_replay = int(cfg["agent_policy"] == "ReplayEgoCarPolicy")
        self.walk_params = walk_params(cfg)      # MdState.walk (all 0 without the walk)
        self.md_config = k


# --------------------------------------------------------------------------------------------------
# Synthetic scenario descriptions (bench / tests): the container holds no ScenarioNet data (nuScenes, Waymo), so scenes
# of the same SHAPE are generated -- a curving multi-lane road, an SDC track along it, vehicles ahead, beside and
# behind it (the ones behind are what ScenarioTrafficManager makes reactive), parked cars, late-appearing and
# vanishing tracks, pedestrians, cones -- in the reference's own description format (scenario_description.py:1-120).
# --------------------------------------------------------------------------------------------------
def _path(rng, n_pts, ds=0.5):
    """a smooth centre line: heading = integral of a slowly varying curvature"""
    amp = rng.uniform(0.004, 0.02)
    wl = rng.uniform(120.0, 300.0)
    ph = rng.uniform(0, 2 * math.pi)
    s = np.arange(n_pts) * ds
    kappa = amp * np.sin(2 * math.pi * s / wl + ph)
    h0 = rng.uniform(-math.pi, math.pi)
    heading = h0 + np.cumsum(kappa) * ds
    x = np.cumsum(np.cos(heading)) * ds + rng.uniform(-500, 500)
    y = np.cumsum(np.sin(heading)) * ds + rng.uniform(-500, 500)
    return s, np.stack([x, y], 1), heading


def _sample(s_axis, xy, heading, s, lateral):
    """pose at arc length s (clamped) with a lateral offset to the right"""
    s = np.clip(s, s_axis[0], s_axis[-1])
    x = np.interp(s, s_axis, xy[:, 0])
    y = np.interp(s, s_axis, xy[:, 1])
    h = np.interp(s, s_axis, heading)
    return x + lateral * np.sin(h), y - lateral * np.cos(h), h


def _track_dict(oid, typ, T, valid, x, y, h, speed, length, width, height):
    v = valid.astype(np.float32)
    pos = np.zeros((T, 3), np.float32)
    pos[:, 0], pos[:, 1] = x * v, y * v
    vel = np.stack([speed * np.cos(h), speed * np.sin(h)], 1).astype(np.float32) * v[:, None]
    return {"type": typ,
            "state": {"position": pos, "heading": (h * v).astype(np.float32), "velocity": vel, "valid": valid.copy(),
                      "length": np.full(T, length, np.float32) * v, "width": np.full(T, width, np.float32) * v,
                      "height": np.full(T, height, np.float32) * v},
            "metadata": {"type": typ, "object_id": str(oid), "track_length": int(T)}}


def _synthetic_lights(seed, n_lights, T, sample, ego_s0):
    """dynamic_map_states with n_lights (0 .. 3) lights, light i on lane "lane<i>" at a stop line 8 .. 32 m ahead of the ego's start,
    cycling green (1.5 s) -> yellow (0.5 s) -> red (1.5 s) from a drawn phase; everything from a RandomState of its own.  New format
    (stop_point at the top level); light 1 in the old one: state["stop_point"] [T, 2] and state["lane"] [T], both 0 in the first
    three frames.  The synthetic ego drives through the stop lines whatever they show."""
    if not 0 <= n_lights <= 3:
        raise ValueError("n_lights={}: 0 .. 3, one light per lane of the synthetic road".format(n_lights))
    rng = np.random.RandomState((int(seed) * 7919 + 104729) % (2 ** 31))
    out = {}
    for i in range(n_lights):
        x, y, _ = sample(np.asarray([ego_s0 + 8.0 + 10.0 * i + rng.uniform(0.0, 4.0)]), (-3.5, 0.0, 3.5)[i])
        phase = int(rng.randint(0, 35))
        at = (np.arange(T) + phase) % 35
        states = np.where(at < 15, "LANE_STATE_GO", np.where(at < 20, "LANE_STATE_CAUTION", "LANE_STATE_STOP")).tolist()
        entry = {"type": "TRAFFIC_LIGHT", "state": {"object_state": states}, "lane": "lane%d" % i,
                 "metadata": {"type": "TRAFFIC_LIGHT", "object_id": "lane%d" % i, "track_length": int(T), "dataset": "synthetic"}}
        if i == 1:
            on = (np.arange(T) >= 3).astype(np.float32)
            entry["state"]["stop_point"] = (np.asarray([[float(x[0]), float(y[0])]], np.float32) * on[:, None]).astype(np.float32)
            entry["state"]["lane"] = on.astype(np.int64)
        else:
            entry["stop_point"] = np.asarray([float(x[0]), float(y[0]), 0.0], np.float32)
        out["lane%d" % i] = entry
    return out


def synthetic_scenario(seed, T=200, n_vehicles=18, n_parked=3, n_pedestrians=2, n_cones=4, n_lights=0):
    rng = np.random.RandomState(seed)
    s_axis, xy, heading = _path(rng, 4000)
    t = np.arange(T) * 0.1
    tracks = {}
    ego_v = rng.uniform(6.0, 11.0)
    ego_s0 = 600.0
    ego_s = ego_s0 + ego_v * t + 0.5 * rng.uniform(-0.15, 0.15) * t * t
    # coordinates relative to the SDC's first position, as the dataset converters deliver them: ScenarioEnv only builds
    # the line bodies whose middle lies within map_region_size / 2 (= 256 m) of the origin (block/base_block.py:481)
    x0_, y0_, _ = _sample(s_axis, xy, heading, np.asarray([ego_s0]), 0.0)
    xy = xy - np.array([float(x0_[0]), float(y0_[0])])
    x, y, h = _sample(s_axis, xy, heading, ego_s, 0.0)
    sp = np.gradient(ego_s, 0.1)
    tracks["0"] = _track_dict("0", "VEHICLE", T, np.ones(T, bool), x, y, h, sp, 4.5, 1.85, 1.5)
    oid = 1
    for i in range(n_vehicles):
        lane = float(rng.choice([-3.5, 0.0, 3.5]))
        behind = i < n_vehicles // 2
        ds0 = rng.uniform(-45.0, -9.0) if behind else rng.uniform(9.0, 70.0)
        if lane == 0.0 and abs(ds0) < 12.0:
            ds0 = math.copysign(12.0, ds0)
        v = max(0.5, ego_v + rng.uniform(-3.0, 3.0))
        s_v = ego_s0 + ds0 + v * t
        x, y, h = _sample(s_axis, xy, heading, s_v, lane)
        valid = np.ones(T, bool)
        r = rng.rand()
        if r < 0.15:
            valid[:int(rng.randint(5, 60 if T > 85 else max(6, T // 3)))] = False          # appears later
        elif r < 0.3:
            valid[int(rng.randint(80 if T > 85 else T // 2, T - 5)):] = False       # vanishes
        length = float(rng.choice([3.9, 4.6, 5.2, 6.0]))
        tracks[str(oid)] = _track_dict(oid, "VEHICLE", T, valid, x, y, h, np.full(T, v), length, 1.9, 1.6)
        oid += 1
    for i in range(n_parked):
        s_p = ego_s0 + rng.uniform(-30.0, 150.0)
        x, y, h = _sample(s_axis, xy, heading, np.full(T, s_p), float(rng.choice([-6.5, 6.5])))
        tracks[str(oid)] = _track_dict(oid, "VEHICLE", T, np.ones(T, bool), x, y, h, np.zeros(T), 4.4, 1.8, 1.5)
        oid += 1
    for i in range(n_pedestrians):
        s_p = ego_s0 + rng.uniform(10.0, 120.0) + rng.uniform(-1.0, 1.0) * t
        x, y, h = _sample(s_axis, xy, heading, s_p, float(rng.choice([-7.5, 7.5])))
        typ = "PEDESTRIAN" if i % 2 == 0 else "CYCLIST"
        tracks[str(oid)] = _track_dict(oid, typ, T, np.ones(T, bool), x, y, h, np.full(T, 1.0), 0.7, 0.7, 1.75)
        oid += 1
    for i in range(n_cones):
        s_p = ego_s0 + 40.0 + 3.0 * i
        x, y, h = _sample(s_axis, xy, heading, np.full(T, s_p), 5.2)
        valid = np.ones(T, bool)
        if i == n_cones - 1:
            valid[10:] = False                                 # a noise object: fewer than MIN_VALID_FRAME_LEN frames
        tracks[str(oid)] = _track_dict(oid, "TRAFFIC_CONE", T, valid, x, y, h, np.zeros(T), 0.4, 0.4, 1.0)
        oid += 1
    # the road itself: three lanes 3.5 m wide around the centre line, solid white edges, broken white separators, a
    # road boundary 0.75 m outside each edge, and (odd seeds) a solid yellow line instead of the right-hand edge
    feats = {}
    s_road = np.arange(ego_s0 - 80.0, ego_s0 + 260.0, 2.0)

    def offset_line(lateral):
        px, py, _ = _sample(s_axis, xy, heading, s_road, lateral)
        return np.stack([px, py, np.zeros_like(px)], 1).astype(np.float32)
    for i, lat in enumerate((-3.5, 0.0, 3.5)):
        feats["lane%d" % i] = {"type": "LANE_SURFACE_STREET", "polyline": offset_line(lat), "entry_lanes": [], "exit_lanes": [],
                               "left_neighbor": [], "right_neighbor": []}
    feats["line_left"] = {"type": "ROAD_LINE_SOLID_SINGLE_WHITE", "polyline": offset_line(-5.25)}
    feats["line_right"] = {"type": "ROAD_LINE_SOLID_SINGLE_YELLOW" if seed % 2 else "ROAD_LINE_SOLID_SINGLE_WHITE",
                           "polyline": offset_line(5.25)}
    feats["sep_left"] = {"type": "ROAD_LINE_BROKEN_SINGLE_WHITE", "polyline": offset_line(-1.75)}
    feats["sep_right"] = {"type": "ROAD_LINE_BROKEN_SINGLE_WHITE", "polyline": offset_line(1.75)}
    feats["edge_left"] = {"type": "ROAD_EDGE_BOUNDARY", "polyline": offset_line(-6.0)}
    feats["edge_right"] = {"type": "ROAD_EDGE_BOUNDARY", "polyline": offset_line(6.0)}
    return {"id": "synthetic-%d" % seed, "version": "metadrive_ped_amd synthetic (MetaDrive v0.4.2.2 scenario format)",
            "length": int(T),
            "metadata": {"ts": t.astype(np.float32), "metadrive_processed": False, "coordinate": "metadrive",
                         "dataset": "synthetic", "seed": int(seed), "sdc_id": "0", "scenario_id": "synthetic-%d" % seed},
            "tracks": tracks,
            "dynamic_map_states": _synthetic_lights(seed, n_lights, T, lambda s, lat: _sample(s_axis, xy, heading, s, lat), ego_s0),
            "map_features": feats}


def synthetic_scenarios(n, seed0=0, **kw):
    return [synthetic_scenario(seed0 + i, **kw) for i in range(n)]
