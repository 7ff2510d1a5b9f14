"""The vector scene observation of scenario mode (config scenario_vector_obs, include/md_scenario_vector_obs.h) on the CPU: the map
piece table the host builds, the route and map rules of the header's gcc build (tests/scenario_vector_obs_host.py) against known
answers on hand-built worlds, a rollout on the oracle against invariants and a numpy restatement, and the config surface."""
import math

import numpy as np
import pytest

import oracle_binding as ob
import scenario_vector_obs_host as sh
from metadrive_ped_amd import abi, scenario as sc
from metadrive_ped_amd.config import SCENARIO_VECTOR_OBS_DEFAULT_CONFIG, check_scenario_vector_obs
from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config, synthetic_scenarios

AGENT = abi.F_ALIVE | abi.F_AGENT


def _line(length, y=0.0, typ="LANE_SURFACE_STREET", step=1.0):
    xs = np.append(np.arange(0.0, length, step), length)
    return {"type": typ, "polyline": np.stack([xs, np.full_like(xs, y), np.zeros_like(xs)], 1)}


# -- the table builder ------------------------------------------------------------------------------------------------------------
def test_a_30_m_lane_gives_16_samples_and_5_pieces_sharing_ends():
    xy, info = sc.scene_map_pieces({"a": _line(30.0)}, 2.0, 4)
    assert xy.shape == (5, 4, 2) and xy.dtype == np.float32 and info.dtype == np.int32
    assert sc.resample_polyline(_line(30.0)["polyline"], 2.0)[:, 0].tolist() == [2.0 * k for k in range(16)]
    assert xy[:, :, 0].tolist() == [[6.0 * q + 2.0 * i for i in range(4)] for q in range(5)]
    assert (xy[1:, 0] == xy[:-1, -1]).all(), "neighbouring pieces share an end point"
    assert info.tolist() == [[0, 0, 4, 0]] * 5


def test_a_7_m_lane_ends_with_a_padded_piece_of_two_points():
    xy, info = sc.scene_map_pieces({"a": _line(7.0, y=1.5)}, 2.0, 4)
    assert xy[:, :, 0].tolist() == [[0.0, 2.0, 4.0, 6.0], [6.0, 7.0, 7.0, 7.0]] and (xy[:, :, 1] == 1.5).all()
    assert info[:, 2].tolist() == [4, 2]


def test_zero_length_steps_are_dropped_and_the_arc_length_follows_the_bends():
    pl = np.asarray([[0, 0], [0, 0], [3, 0], [3, 0], [3, 4]], np.float64)
    pts = sc.resample_polyline(pl, 2.0)
    assert pts.tolist() == [[0, 0], [2, 0], [3, 1], [3, 3], [3, 4]]
    assert sc.resample_polyline(np.asarray([[1.0, 1.0], [1.0, 1.0 + 1e-7]]), 2.0) is None


def test_type_codes_classes_and_skipped_features():
    names = sc.MAP_FEATURE_TYPES
    assert len(names) == len(set(names)) == 17
    feats = {}
    for i, t in enumerate(names):
        feats["f%d" % i] = _line(3.0, y=float(i), typ=t)
    feats["one_point"] = {"type": "LANE_SURFACE_STREET", "polyline": np.zeros((1, 3))}
    feats["crosswalk"] = {"type": "CROSSWALK", "polygon": np.zeros((4, 3))}
    feats["sidewalk"] = {"type": "ROAD_EDGE_SIDEWALK", "polygon": np.zeros((4, 3))}
    feats["bump"] = {"type": "SPEED_BUMP", "polygon": np.zeros((4, 3))}
    feats["stop"] = {"type": "STOP_SIGN", "position": np.zeros(3)}
    feats["drive"] = {"type": "DRIVEWAY", "polyline": _line(5.0)["polyline"]}
    feats["late"] = _line(3.0, y=50.0, typ="ROAD_EDGE_MEDIAN")
    xy, info = sc.scene_map_pieces(feats, 2.0, 4)
    assert info[:, 1].tolist() == list(range(17)) + [16]
    assert info[:, 0].tolist() == [0] * 5 + [1] * 9 + [2] * 3 + [2]
    assert info[:, 3].tolist() == list(range(17)) + [23], "the ordinal counts every feature of the dict"
    for t in ("LANE_SURFACE_STREET", "LANE_FREEWAY", "LANE_BIKE_LANE"):
        assert sc.map_feature_class(names.index(t)) == sc.MAP_CLASS_LANE
    for t in ("UNKNOWN_LINE", "ROAD_LINE_BROKEN_SINGLE_WHITE", "ROAD_LINE_PASSING_DOUBLE_YELLOW"):
        assert sc.map_feature_class(names.index(t)) == sc.MAP_CLASS_LINE
    for t in ("UNKNOWN", "ROAD_EDGE_BOUNDARY", "ROAD_EDGE_MEDIAN"):
        assert sc.map_feature_class(names.index(t)) == sc.MAP_CLASS_EDGE


def test_tables_offsets_and_balls():
    a = sc.scene_map_pieces({"a": _line(30.0), "b": _line(7.0, y=3.0, typ="ROAD_EDGE_BOUNDARY")}, 2.0, 4)
    b = sc.scene_map_pieces({}, 2.0, 4)
    c = sc.scene_map_pieces({"c": _line(9.0, y=-900.0)}, 2.0, 4)
    t = sc.map_piece_tables([a, b, c], 4)
    assert t["map_off"].tolist() == [0, 7, 7, 9] and t["max_pieces"] == 7 and t["map_off"].dtype == np.int32
    assert t["map_xy"].shape == (9, 4, 2) and t["map_info"].shape == (9, 4) and t["map_ball"].shape == (9, 4)
    ball, xy = t["map_ball"].astype(np.float64), t["map_xy"].astype(np.float64)
    far = np.hypot(xy[:, :, 0] - ball[:, None, 0], xy[:, :, 1] - ball[:, None, 1]).max(1)
    assert (ball[:, 2] >= far + 1e-3).all() and (ball[:, 2] <= far + 0.01).all() and (ball[:, 3] == 0).all()
    empty = sc.map_piece_tables([b], 4)
    assert empty["map_off"].tolist() == [0, 0] and empty["max_pieces"] == 0 and len(empty["map_xy"]) == 1


def test_a_scene_past_the_piece_ceiling_is_refused_by_both_keys():
    assert abi.MD_SVO_MAX_PIECES == 4096
    feats = {"f%d" % i: _line(1000.0, y=float(i), step=50.0) for i in range(9)}
    ok = sc.map_piece_tables([sc.scene_map_pieces(feats, 2.0, 8)], 8)
    assert ok["max_pieces"] == 9 * 72
    with pytest.raises(ValueError) as err:
        sc.map_piece_tables([sc.scene_map_pieces(feats, 2.0, 2)], 2)          # 9 x 500 pieces
    assert "map_spacing" in str(err.value) and "piece_points" in str(err.value) and "4500" in str(err.value)
    # ... and through the host scene
    scs = synthetic_scenarios(1, T=20)
    scs[0]["map_features"] = feats
    cfg = make_scenario_config(dict(num_envs=1, num_scenarios=1, scenario_vector_obs=dict(piece_points=2)))
    with pytest.raises(ValueError, match="map_spacing"):
        ScenarioHostScene(cfg, scs)


# -- the route ----------------------------------------------------------------------------------------------------------------------
def _straight(length=100.0, cap=8):
    return sh.trajectory_world([(float(x), 0.0) for x in np.arange(0.0, length + 0.5, 1.0)], cap)


def _route(vo, w, s, k):
    hv = sh.HostScenarioVectorObs(dict(vo, num_pieces=0), 1, k.cap).run(w, s, k)
    return hv.out("route")[0], hv.out("route_mask")[0], hv


def test_route_rows_on_a_straight_trajectory():
    w, s, k, st, _ = _straight()
    sh.put(st, 0, 10.0, 0.5, 0.0, flags=AGENT)
    route, mask, hv = _route(dict(route_points=8, route_spacing=4.0), w, s, k)
    assert mask.tolist() == [1] * 8
    assert route.tolist() == [[4.0 * (m + 1), -0.5, 1.0, 0.0] for m in range(8)]
    assert hv.out("ego")[0, 0].tolist() == [0.0, 0.0, 1.0, 0.0] and hv.out("ego_mask")[0].tolist() == [1, 0, 0, 0, 0]


def test_route_rows_are_masked_exactly_beyond_the_trajectory_s_end():
    w, s, k, st, _ = _straight(100.0)
    sh.put(st, 0, 80.0, 0.0, 0.0, flags=AGENT)
    route, mask, _ = _route(dict(route_points=8, route_spacing=4.0), w, s, k)
    assert mask.tolist() == [1] * 5 + [0] * 3, "84 .. 100 are on the trajectory (the end itself included), 104 is not"
    assert route[4].tolist() == [20.0, 0.0, 1.0, 0.0] and not route[5:].any()
    # an observer behind the start is clipped onto it; one past the end has no route left
    sh.put(st, 0, -7.0, 0.0, 0.0, flags=AGENT)
    route, mask, _ = _route(dict(route_points=3, route_spacing=4.0), w, s, k)
    assert route[:, 0].tolist() == [11.0, 15.0, 19.0] and mask.all()
    sh.put(st, 0, 130.0, 0.0, 0.0, flags=AGENT)
    route, mask, _ = _route(dict(route_points=3, route_spacing=4.0), w, s, k)
    assert not mask.any() and not route.any()


def test_the_route_s_frame_turns_with_the_ego():
    w, s, k, st, _ = _straight()
    sh.put(st, 0, 10.0, 0.5, math.pi / 2, flags=AGENT)       # facing +y: the trajectory runs to its right
    route, mask, _ = _route(dict(route_points=4, route_spacing=4.0), w, s, k)
    want = np.asarray([[-0.5, -4.0 * (m + 1), 0.0, -1.0] for m in range(4)], np.float32)
    assert mask.all() and np.abs(route - want).max() < 1e-5, route


def test_the_route_follows_a_bend_and_an_invalid_observer_gets_nothing():
    pts = [(float(x), 0.0) for x in range(0, 21)] + [(20.0, float(y)) for y in range(1, 21)]
    w, s, k, st, _ = sh.trajectory_world(pts)
    sh.put(st, 0, 15.0, 0.0, 0.0, flags=AGENT)
    route, mask, _ = _route(dict(route_points=4, route_spacing=4.0), w, s, k)
    want = [[4.0, 0.0, 1.0, 0.0], [5.0, 3.0, 0.0, 1.0], [5.0, 7.0, 0.0, 1.0], [5.0, 11.0, 0.0, 1.0]]
    assert np.abs(route - np.asarray(want, np.float32)).max() < 1e-5 and mask.all()
    st["shape"][0]["flags"] = 0
    hv = sh.HostScenarioVectorObs(dict(num_pieces=0), 1, k.cap).run(w, s, k)
    assert not any(v.any() for v in hv.outputs().values())


# -- the map selection --------------------------------------------------------------------------------------------------------------
def _map(features, vo, x=0.0, y=0.0, heading=0.0):
    vo = check_scenario_vector_obs(dict(dict(route_points=0), **vo))
    w, s, k, st, _ = _straight()
    sh.put(st, 0, x, y, heading, flags=AGENT)
    pieces = sh.pieces_of(features, vo["map_spacing"], vo["piece_points"])
    hv = sh.HostScenarioVectorObs(vo, 1, k.cap, pieces).run(w, s, k)
    return hv.out("map")[0], hv.out("map_mask")[0], hv.out("map_meta")[0], pieces


def test_map_pieces_come_in_the_order_of_distance_then_index():
    feats = {"far": _line(6.0, y=9.0), "near": _line(6.0, y=2.0, typ="ROAD_LINE_SOLID_SINGLE_WHITE"),
             "twin": _line(6.0, y=2.0, typ="ROAD_EDGE_BOUNDARY"), "mid": _line(6.0, y=-4.0)}
    m, mask, meta, _ = _map(feats, dict(num_pieces=6, piece_points=4))
    assert meta[:, 3].tolist() == [4.0, 4.0, 16.0, 81.0, 0.0, 0.0], "two identical polylines tie by index; two ranks stay empty"
    assert meta[:, 0].tolist() == [1.0, 2.0, 0.0, 0.0, 0.0, 0.0]
    assert meta[:, 1].tolist() == [float(sc.MAP_FEATURE_TYPES.index("ROAD_LINE_SOLID_SINGLE_WHITE")),
                                   float(sc.MAP_FEATURE_TYPES.index("ROAD_EDGE_BOUNDARY")), 0.0, 0.0, 0.0, 0.0]
    assert mask.tolist() == [[1] * 4] * 4 + [[0] * 4] * 2 and not m[4:].any()
    assert m[0].tolist() == [[0.0, 2.0], [2.0, 2.0], [4.0, 2.0], [6.0, 2.0]] and m[0].tolist() == m[1].tolist()
    # fewer ranks than candidates: the nearest are kept
    m2, _, meta2, _ = _map(feats, dict(num_pieces=2, piece_points=4))
    assert meta2.tolist() == meta[:2].tolist() and m2.tolist() == m[:2].tolist()


def test_the_radius_cut_is_inclusive():
    feats = {"at": _line(6.0, y=3.0), "past": _line(6.0, y=3.0001)}
    _, mask, meta, _ = _map(feats, dict(num_pieces=4, piece_points=4, map_radius=3.0))
    assert meta[:, 3].tolist() == [9.0, 0.0, 0.0, 0.0] and mask.sum() == 4


def test_the_point_mask_of_a_padded_piece_and_the_ego_frame():
    feats = {"a": _line(7.0, y=1.0)}
    m, mask, meta, _ = _map(feats, dict(num_pieces=2, piece_points=4), x=7.0, y=0.0, heading=math.pi / 2)
    assert meta[:, 2].tolist() == [2.0, 4.0] and meta[:, 3].tolist() == [1.0, 2.0]
    assert mask.tolist() == [[1, 1, 0, 0], [1, 1, 1, 1]]
    assert not m[0, 2:].any(), "a padded point is masked and zero"
    want = np.asarray([[1.0, 1.0], [1.0, 0.0]], np.float32)      # (6, 1) and (7, 1) seen from (7, 0) facing +y: forward 1, left 1 / 0
    assert np.abs(m[0, :2] - want).max() < 1e-6


def test_the_numpy_restatement_agrees_on_a_dense_scene():
    feats = synthetic_scenarios(1, T=20)[0]["map_features"]
    for vo in (dict(sh.SMALL), dict(num_pieces=64, piece_points=16), {}):
        vo = check_scenario_vector_obs(vo)
        m, mask, meta, pieces = _map(feats, vo, x=3.0, y=-2.0, heading=0.7)
        want = sh.select_pieces(pieces, 0, 3.0, -2.0, np.float32(math.cos(0.7)), np.float32(math.sin(0.7)), vo["map_radius"],
                                vo["num_pieces"], vo["piece_points"])
        assert meta.tobytes() == want[2].tobytes() and mask.tobytes() == want[1].tobytes() and m.tobytes() == want[0].tobytes()
        assert mask[:, 0].sum() == min(vo["num_pieces"], int((meta[:, 2] > 0).sum())) and mask[0, 0]


# -- a rollout on the oracle ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rollout():
    """4 synthetic scenes of 40 frames through ScenarioHostScene and the oracle, 30 steps: per step the oracle's state (copies) and
    the host build's outputs and history"""
    E = 4
    vo = dict(sh.SMALL, num_agents=6, num_pieces=5)
    cfg = make_scenario_config(dict(num_envs=E, num_scenarios=E, horizon=400, auto_reset=False, scenario_vector_obs=vo))
    host = ScenarioHostScene(cfg, synthetic_scenarios(E, T=40))
    o = ob.OracleWorld(host)
    o.set_tracks(host.tracks["shape"], host.tracks["dyn"])
    hv = sh.HostScenarioVectorObs(cfg["scenario_vector_obs"], E, host.cap, host.map_pieces)
    frames = []

    def observe():
        w, s, k, keep = sh.structs_of(host, o.state)
        hv.run(w, s, k)
        frames.append(dict(shape=o.state["shape"].reshape(E, host.cap).copy(), out=hv.outputs(), hist=hv.history()))
    o.reset()
    observe()
    act = np.zeros((E, 1, 2), np.float32)
    act[:, 0, 1] = 0.3
    for t in range(30):
        o.step(act)
        observe()
    return dict(cfg=cfg, host=host, frames=frames, hv=hv)


def test_rollout_route_points_lie_on_the_reference_polyline(rollout):
    host, vo = rollout["host"], rollout["cfg"]["scenario_vector_obs"]
    arr = host.world.arrays
    seen = 0
    for fr in rollout["frames"]:
        for e in range(host.E):
            me = fr["shape"][e, 0]
            a, b = int(arr["poly_off"][e * host.cap]), int(arr["poly_off"][e * host.cap + 1])
            g = arr["segs"][a:b]
            route, mask = fr["out"]["route"][e].astype(np.float64), fr["out"]["route_mask"][e]
            along = []
            for m in np.nonzero(mask)[0]:
                # back to the world frame, then the distance to the nearest piece and the arc length there
                x = me["cx"] + route[m, 0] * me["c"] - route[m, 1] * me["s"]
                y = me["cy"] + route[m, 0] * me["s"] + route[m, 1] * me["c"]
                t = np.clip((x - g["sx"]) * g["dx"] + (y - g["sy"]) * g["dy"], 0.0, g["len"])
                d = np.hypot(x - (g["sx"] + t * g["dx"]), y - (g["sy"] + t * g["dy"]))
                i = int(np.argmin(d))
                assert d[i] < 1e-3, (e, m, d[i])
                along.append(float(g["cum"][i] + t[i]))
                assert abs(math.hypot(route[m, 2], route[m, 3]) - 1.0) < 1e-5
                seen += 1
            assert mask.tolist() == sorted(mask.tolist(), reverse=True), "the valid rows come first"
            if len(along) > 1:
                assert np.abs(np.diff(along) - vo["route_spacing"]).max() < 2e-3, along
    assert seen > 100


def test_rollout_map_selection_equals_the_numpy_restatement(rollout):
    host, vo, taken = rollout["host"], rollout["cfg"]["scenario_vector_obs"], 0
    for fr in rollout["frames"]:
        for e in range(host.E):
            me = fr["shape"][e, 0]
            want = sh.select_pieces(host.map_pieces, e, me["cx"], me["cy"], me["c"], me["s"], vo["map_radius"], vo["num_pieces"],
                                    vo["piece_points"])
            for name, w in zip(("map", "map_mask", "map_meta"), want):
                assert fr["out"][name][e].tobytes() == w.tobytes(), (e, name)
            taken += int(want[1][:, 0].sum())
    assert taken == len(rollout["frames"]) * host.E * vo["num_pieces"]


def test_rollout_a_reset_leaves_one_held_frame_and_the_history_fills(rollout):
    first, later = rollout["frames"][0], rollout["frames"][5]
    assert (first["hist"]["cursor"][:, 1] == 1).all() and first["out"]["ego_mask"].tolist() == [[1, 0, 0]] * 4
    assert (first["out"]["agents_mask"][:, :, 1:] == 0).all() and first["out"]["agents_mask"][:, :, 0].any()
    assert (later["hist"]["cursor"][:, 1] == 3).all() and later["out"]["ego_mask"].tolist() == [[1, 1, 1]] * 4


def test_rollout_a_late_track_has_no_frames_from_before_it_appeared(rollout):
    """a slot that was absent in the previous frame and is present now, seen as a neighbour: only its newest frame is valid"""
    host, late = rollout["host"], 0
    frames = rollout["frames"]
    vo = dict(rollout["cfg"]["scenario_vector_obs"], radius=1000.0, num_agents=16, num_pieces=0, route_points=0)
    hv = sh.HostScenarioVectorObs(vo, host.E, host.cap)
    E, cap = host.E, host.cap
    for t, fr in enumerate(frames):
        state = dict(shape=fr["shape"].reshape(-1), dyn=np.zeros(E * cap, abi.DYN_DT), nav=np.zeros(E * cap, abi.NAV_DT))
        state["nav"]["steps"][::cap] = t
        w, s, k, keep = sh.structs_of(host, state)
        hv.run(w, s, k)
        if t == 0:
            continue
        now = (fr["shape"]["flags"] & abi.F_ALIVE) != 0
        before = (frames[t - 1]["shape"]["flags"] & abi.F_ALIVE) != 0
        masks, me = hv.out("agents_mask"), fr["shape"][:, 0]
        for e, j in zip(*np.nonzero(now & ~before)):
            d2 = (np.float32(fr["shape"][e, j]["cx"]) - me["cx"][e]) ** 2 + (np.float32(fr["shape"][e, j]["cy"]) - me["cy"][e]) ** 2
            others = [(np.float32(q["cx"] - me["cx"][e]) ** 2 + np.float32(q["cy"] - me["cy"][e]) ** 2, i)
                      for i, q in enumerate(fr["shape"][e]) if i and (q["flags"] & abi.F_ALIVE)]
            rank = sorted(others).index((d2, j)) if (d2, j) in others else None
            if rank is not None and rank < 16:
                assert masks[e, rank].tolist() == [1, 0, 0], (t, e, j)
                late += 1
    assert late > 0, "the synthetic scenes hold tracks that appear after frame 0"


# -- the config ---------------------------------------------------------------------------------------------------------------------
def test_defaults_ranges_and_unknown_keys():
    assert SCENARIO_VECTOR_OBS_DEFAULT_CONFIG == dict(num_agents=8, history=5, radius=50.0, max_jump=8.0, route_points=16, route_spacing=4.0,
                                                      num_pieces=32, piece_points=8, map_radius=50.0, map_spacing=2.0)
    assert make_scenario_config({})["scenario_vector_obs"] is None
    assert make_scenario_config(dict(scenario_vector_obs={}))["scenario_vector_obs"] == SCENARIO_VECTOR_OBS_DEFAULT_CONFIG
    got = check_scenario_vector_obs(dict(num_pieces=0, map_radius=30))
    assert got["num_pieces"] == 0 and got["map_radius"] == 30.0 and isinstance(got["map_radius"], float)
    for key, lo, hi in (("num_agents", 1, 16), ("history", 1, 8), ("route_points", 0, 32), ("num_pieces", 0, 64), ("piece_points", 2, 16)):
        check_scenario_vector_obs({key: lo}), check_scenario_vector_obs({key: hi})
        for bad in (lo - 1, hi + 1, 2.0, True, "3"):
            with pytest.raises(ValueError, match=r"scenario_vector_obs\['%s'\]" % key):
                check_scenario_vector_obs({key: bad})
    for key in ("radius", "max_jump", "route_spacing", "map_radius", "map_spacing"):
        for bad in (0, -1.0, float("nan"), None, True):
            with pytest.raises(ValueError, match=r"scenario_vector_obs\['%s'\]" % key):
                check_scenario_vector_obs({key: bad})
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['num_lanes'\]"):
        check_scenario_vector_obs(dict(num_lanes=4))
    with pytest.raises(ValueError, match="scenario_vector_obs=3"):
        make_scenario_config(dict(scenario_vector_obs=3))


def test_the_key_belongs_to_the_scenario_envs_and_vector_obs_stays_refused():
    from metadrive_ped_amd.config import make_config
    with pytest.raises(KeyError):
        make_config(dict(scenario_vector_obs={}))
    with pytest.raises(NotImplementedError, match="vector_obs in BatchedScenarioEnv is not built"):
        make_scenario_config(dict(vector_obs={}))


def test_the_env_s_spec_and_the_refusal_without_the_key():
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    env = BatchedScenarioEnv(dict(num_envs=2, num_scenarios=2, scenario_vector_obs=dict(sh.SMALL)), scenarios=synthetic_scenarios(2, T=20))
    spec = env.vector_obs_spec()
    assert list(spec) == list(abi.SCENARIO_VECTOR_OBS_OUTPUTS)
    assert spec["agents"] == ((2, 3, 3, 4), np.float32) and spec["map"] == ((2, 3, 3, 2), np.float32)
    assert spec["map_mask"] == ((2, 3, 3), np.uint8) and spec["map_meta"] == ((2, 3, 4), np.float32) and spec["route_mask"] == ((2, 5), np.uint8)
    with pytest.raises(RuntimeError, match="reset"):
        env.vector_obs()
    off = BatchedScenarioEnv(dict(num_envs=2, num_scenarios=2), scenarios=synthetic_scenarios(2, T=20))
    for call in (off.vector_obs, off.vector_obs_spec):
        with pytest.raises(RuntimeError, match="scenario_vector_obs"):
            call()


def test_the_host_scene_builds_the_table_only_with_the_key():
    scs = synthetic_scenarios(2, T=20)
    off = ScenarioHostScene(make_scenario_config(dict(num_envs=2, num_scenarios=2)), scs)
    assert off.map_pieces is None
    on = ScenarioHostScene(make_scenario_config(dict(num_envs=2, num_scenarios=2, scenario_vector_obs=dict(sh.SMALL))), scs)
    assert on.map_pieces["map_off"].shape == (3, ) and on.map_pieces["max_pieces"] > 700
    none = ScenarioHostScene(make_scenario_config(dict(num_envs=2, num_scenarios=2, scenario_vector_obs=dict(num_pieces=0))), scs)
    assert none.map_pieces is None
