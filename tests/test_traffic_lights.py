"""The traffic lights of scenario mode (include/md_traffic_lights.h, config traffic_lights) without a GPU: the status map, the host
tables built from scenario descriptions, and the rule -- the gcc build of the header (tests/traffic_lights_host.py) on placed states
against a float64 numpy restatement whose box test is tests/contact_ref.py's, the frame a light shows and the frame it acts with, the
selection of the nearest lights -- and the config keys."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import traffic_lights_host as th
from metadrive_ped_amd import abi
from metadrive_ped_amd import scenario as sc
from metadrive_ped_amd.scenario import make_scenario_config, synthetic_scenario

G, Y, R, U = abi.TL_GREEN, abi.TL_YELLOW, abi.TL_RED, abi.TL_UNKNOWN


# -- 1. the status map ---------------------------------------------------------------------------------------------------------------
STATUS = [("LANE_STATE_UNKNOWN", U), ("LANE_STATE_ARROW_STOP", R), ("LANE_STATE_ARROW_CAUTION", Y), ("LANE_STATE_ARROW_GO", G),
          ("LANE_STATE_STOP", R), ("LANE_STATE_CAUTION", Y), ("LANE_STATE_GO", G), ("LANE_STATE_FLASHING_STOP", U),
          ("LANE_STATE_FLASHING_CAUTION", Y), ("TRAFFIC_LIGHT_GREEN", G), ("TRAFFIC_LIGHT_RED", R), ("TRAFFIC_LIGHT_YELLOW", Y),
          ("TRAFFIC_LIGHT_UNKNOWN", U), (None, U), ("LANE_STATE_PURPLE", U)]


@pytest.mark.parametrize("status,code", STATUS)
def test_status_map(status, code):
    assert (U, G, Y, R) == (0, 1, 2, 3)
    assert sc.light_status_code(status) == code
    if status is not None:
        assert sc.light_status_code(np.str_(status)) == code and sc.light_status_code(status.encode()) == code


# -- 2. tables from descriptions -----------------------------------------------------------------------------------------------------
def _lane(points, typ="LANE_SURFACE_STREET"):
    return {"type": typ, "polyline": np.asarray([(x, y, 0.0) for x, y in points], np.float32)}


BENT = [(0.0, 0.0), (2.0, 0.0), (4.0, 0.0), (6.0, 0.0), (8.0, 0.0), (10.0, 0.0), (10.0, 2.0), (10.0, 4.0), (10.0, 6.0), (10.0, 8.0), (10.0, 10.0)]


def _new(lane, xy, states, typ="TRAFFIC_LIGHT"):
    return {"type": typ, "lane": lane, "stop_point": np.asarray([xy[0], xy[1], 0.0], np.float32), "state": {"object_state": list(states)},
            "metadata": {}}


def _old(lane_frames, rows, states):
    return {"type": "TRAFFIC_LIGHT", "metadata": {},
            "state": {"object_state": list(states), "lane": np.asarray(lane_frames), "stop_point": np.asarray(rows, np.float32)}}


def _description(lights, feats=None):
    return {"map_features": feats if feats is not None else {"7": _lane(BENT), "8": _lane([(0.0, 5.0), (20.0, 5.0)])},
            "dynamic_map_states": lights}


def test_new_and_old_position_formats_and_the_ordinal():
    rows = [(0.0, 0.0), (0.0, 0.0), (3.0, 5.0), (4.0, 5.0)]
    d = _description({7: _new("ignored", (10.0, 8.0), ["LANE_STATE_STOP", "LANE_STATE_GO", None]),
                      "8": _old([0, 0, 8, 8], rows, ["LANE_STATE_CAUTION"] * 4)})
    box, status, ids = sc.scene_traffic_lights(d)
    assert ids == [7, "8"], "the keys as the description has them, in the dict's order"
    assert box.dtype == np.float32 and box.shape == (2, 8)
    assert box[0, :2].tolist() == [10.0, 8.0], "new format: stop_point[:2] of the entry; the lane is the FEATURE str(key), not the lane field"
    assert box[1, :2].tolist() == [3.0, 5.0], "old format: the row of the first frame whose lane is not 0"
    assert [s.tolist() for s in status] == [[R, G, U], [Y] * 4] and all(s.dtype == np.uint8 for s in status)
    t = sc.traffic_light_tables([(box, status, ids)])
    assert t["tl_off"].tolist() == [0, 2] and t["tl_info"].tolist() == [[0, 3, 0, 0], [3, 4, 1, 0]]
    assert t["tl_status"][:7].tolist() == [R, G, U, Y, Y, Y, Y] and t["max_scene_lights"] == 2 and t["ids"] == [[7, "8"]]
    assert t["tl_box"].dtype == np.float32 and t["tl_info"].dtype == np.int32 and t["tl_status"].dtype == np.uint8


def test_a_light_whose_lane_array_is_all_zero_takes_the_last_row():
    d = _description({"8": _old([0, 0, 0], [(1.0, 5.0), (2.0, 5.0), (7.0, 5.0)], ["LANE_STATE_GO"] * 3)})
    assert sc.scene_traffic_lights(d)[0][0, :2].tolist() == [7.0, 5.0]


def test_a_light_on_a_missing_lane_is_skipped_or_refused():
    lights = {"7": _new("7", (10.0, 8.0), ["LANE_STATE_GO"]), "99": _new("99", (0.0, 0.0), ["LANE_STATE_STOP"]),
              "edge": _new("edge", (1.0, 1.0), ["LANE_STATE_STOP"]), "8": _new("8", (5.0, 5.0), ["LANE_STATE_STOP"])}
    feats = {"7": _lane(BENT), "8": _lane([(0.0, 5.0), (20.0, 5.0)]), "edge": _lane([(0.0, 9.0), (20.0, 9.0)], "ROAD_EDGE_BOUNDARY")}
    box, status, ids = sc.scene_traffic_lights(_description(lights, feats), True)
    assert ids == ["7", "8"], "no such feature, and a feature that is no lane"
    t = sc.traffic_light_tables([(box, status, ids)])
    assert t["tl_info"][:, 2].tolist() == [0, 1], "the ordinal counts the kept lights"
    with pytest.raises(ValueError) as err:
        sc.scene_traffic_lights(_description(lights, feats), False)
    assert str(err.value) == "Can not find lane for this traffic light. Set skip_missing_light=True for skipping missing light!"


def test_an_entry_that_is_no_light_is_refused():
    with pytest.raises(ValueError, match="Can not handle STOP_SIGN"):
        sc.scene_traffic_lights(_description({"7": _new("7", (1.0, 0.0), ["LANE_STATE_GO"], typ="STOP_SIGN")}))


def test_the_wall_heads_where_the_lane_heads_at_five_metres():
    box, _, _ = sc.scene_traffic_lights(_description({"7": _new("7", (10.0, 8.0), ["LANE_STATE_GO"])}))
    lane = sc.PolyLine(BENT)
    at5, at_stop = lane.heading_at(5.0), lane.heading_at(lane.local_coordinates((10.0, 8.0))[0])
    assert at5 == 0.0 and abs(at_stop - 0.5 * math.pi) < 1e-12, "the lane turns left between 5 m and the stop point"
    assert box[0, 2:6].tolist() == [1.0, 0.0, 0.125, 3.0], "cos, sin of the heading at PLACE_LONGITUDE; 0.25 m along it, 6 m across"
    lib = th.lib()
    assert [lib.hx_tl_constant(i) for i in range(3)] == [sc.AIR_WALL_LENGTH, sc.LIGHT_LANE_WIDTH, sc.PLACE_LONGITUDE] == [0.25, 6.0, 5.0]
    assert (th.HL, th.HW) == (0.5 * sc.AIR_WALL_LENGTH, 0.5 * sc.LIGHT_LANE_WIDTH)


def test_the_scene_ceiling_and_an_empty_scene():
    box = np.zeros((1025, 8), np.float32)
    with pytest.raises(ValueError, match="MD_TL_MAX_SCENE_LIGHTS=1024"):
        sc.traffic_light_tables([(box, [np.zeros(1, np.uint8)] * 1025, list(range(1025)))])
    t = sc.traffic_light_tables([(box[:0], [], []), (box[:1024], [np.zeros(1, np.uint8)] * 1024, list(range(1024)))])
    assert t["tl_off"].tolist() == [0, 0, 1024] and t["max_scene_lights"] == 1024
    empty = sc.traffic_light_tables([(box[:0], [], [])])
    assert empty["tl_off"].tolist() == [0, 0] and len(empty["tl_box"]) == 1 and len(empty["tl_info"]) == 1 and len(empty["tl_status"]) == 1


def _same(a, b, where=""):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], where + "/" + str(k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


def test_the_synthetic_scenario_without_lights_is_what_it_was():
    plain = synthetic_scenario(5, T=40)
    assert plain["dynamic_map_states"] == {}
    _same(plain, synthetic_scenario(5, T=40, n_lights=0))
    lit = synthetic_scenario(5, T=40, n_lights=3)
    for key in ("tracks", "map_features", "metadata", "length", "id"):       # the lights draw from a stream of their own
        _same(plain[key], lit[key], key)
    lights = lit["dynamic_map_states"]
    assert list(lights) == ["lane0", "lane1", "lane2"] and "stop_point" in lights["lane1"]["state"] and "stop_point" in lights["lane0"]
    assert lights["lane1"]["state"]["stop_point"].shape == (40, 2) and not lights["lane1"]["state"]["lane"][:3].any()
    box, status, ids = sc.scene_traffic_lights(lit)
    assert ids == ["lane0", "lane1", "lane2"] and all(len(s) == 40 and set(s.tolist()) <= {G, Y, R} for s in status)
    ego = plain["tracks"]["0"]["state"]["position"][0, :2]
    ahead = np.hypot(*(box[:, :2] - ego).T)
    assert (ahead > 7.0).all() and (ahead < 34.0).all(), "stop lines 8 .. 32 m ahead of the ego's start, on lanes 3.5 m apart"
    with pytest.raises(ValueError, match="n_lights=4"):
        synthetic_scenario(5, T=40, n_lights=4)


def test_the_host_scene_carries_the_tables_only_with_the_key():
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    scenes = [synthetic_scenario(5, T=30, n_lights=3), synthetic_scenario(6, T=30, n_lights=1)]
    host = BatchedScenarioEnv(dict(num_envs=2, num_scenarios=2, traffic_lights={}), scenarios=scenes)._build_host()
    assert host.traffic_lights["tl_off"].tolist() == [0, 3, 4] and host.traffic_light_ids == [["lane0", "lane1", "lane2"], ["lane0"]]
    off = BatchedScenarioEnv(dict(num_envs=2, num_scenarios=2), scenarios=scenes)._build_host()
    assert off.traffic_lights is None and off.traffic_light_ids is None


def test_a_dataset_folder_s_lights_arrive_in_the_tables(tmp_path):
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    from metadrive_ped_amd.scenario_data import write_dataset
    scenes = [synthetic_scenario(5, T=30, n_lights=3), synthetic_scenario(6, T=30, n_lights=2)]
    write_dataset(str(tmp_path), scenes)
    cfg = dict(num_envs=2, num_scenarios=2, traffic_lights={})
    read = BatchedScenarioEnv(dict(cfg, data_directory=str(tmp_path)))._build_host().traffic_lights
    handed = BatchedScenarioEnv(cfg, scenarios=scenes)._build_host().traffic_lights
    assert read["tl_off"].tolist() == [0, 3, 5] and read["ids"] == handed["ids"]
    for k in abi.TRAFFIC_LIGHTS_TABLES:
        assert read[k].tobytes() == handed[k].tobytes(), k


def test_a_curriculum_s_sorted_pool_keeps_every_scene_s_own_lights():
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    scenes = [synthetic_scenario(20 + i, T=30, n_lights=i % 4) for i in range(4)]
    lights_of = {s["id"]: i % 4 for i, s in enumerate(scenes)}
    host = BatchedScenarioEnv(dict(num_envs=2, num_scenarios=4, walk_scenarios=True, sequential_seed=True, curriculum_level=2,
                                   traffic_lights={}), scenarios=scenes)._build_host()
    assert sorted(host.scenario_ids) == sorted(lights_of) and host.scenario_ids != [s["id"] for s in scenes], "the pool is sorted by difficulty"
    assert [len(ids) for ids in host.traffic_light_ids] == [lights_of[i] for i in host.scenario_ids]
    assert np.diff(host.traffic_lights["tl_off"]).tolist() == [lights_of[i] for i in host.scenario_ids]


# -- 3. placed states: the host build against float64 --------------------------------------------------------------------------------
# Every case keeps at least 1e-3 m (contact_ref.EPS) between "touching" and its pose: ref_agent_light reports it as decided, and
# float32 and float64 then agree on every boolean.  Wall: 0.125 m x 3 m half extents; ego: 2.25 m x 0.9 m.
_N45 = (math.cos(0.25 * math.pi), math.sin(0.25 * math.pi))
_TOUCH45 = (th.EGO_HL + th.EGO_HW) * _N45[0] + th.HL         # the ego's reach along the wall's normal + the wall's half length
PLACED = [
    ("across a red wall", [(10.0, 5.0, 0.0, [R])], (10.0, 5.0, 0.0), True, abi.TL_BIT_RED),
    ("1 cm short of it", [(10.0, 5.0, 0.0, [R])], (10.0 - th.HL - th.EGO_HL - 0.01, 5.0, 0.0), True, 0),
    ("1 cm into it", [(10.0, 5.0, 0.0, [R])], (10.0 - th.HL - th.EGO_HL + 0.01, 5.0, 0.0), True, abi.TL_BIT_RED),
    ("a wall rotated 45 degrees, 1.2 cm into it", [(0.0, 0.0, 0.25 * math.pi, [Y])],
     ((_TOUCH45 - 0.012) * _N45[0], (_TOUCH45 - 0.012) * _N45[1], 0.0), True, abi.TL_BIT_YELLOW),
    ("a wall rotated 45 degrees, 1.8 cm short", [(0.0, 0.0, 0.25 * math.pi, [Y])],
     ((_TOUCH45 + 0.018) * _N45[0], (_TOUCH45 + 0.018) * _N45[1], 0.0), True, 0),
    ("on a red and a green wall at once", [(0.0, 0.0, 0.0, [R]), (1.0, 0.0, 0.0, [G])], (0.5, 0.2, 0.1), True,
     abi.TL_BIT_RED | abi.TL_BIT_GREEN),
    ("an unknown light overlapped", [(0.0, 0.0, 0.0, [U])], (0.0, 0.0, 0.0), True, 0),
    ("the observer absent", [(0.0, 0.0, 0.0, [R])], (0.0, 0.0, 0.0), False, 0),
]


@pytest.mark.parametrize("name,lights,ego,present,bits", PLACED, ids=[p[0] for p in PLACED])
def test_placed_states(name, lights, ego, present, bits):
    out, tables, st = th.run_world(lights, ego, clock=1, present=present)
    want, decided = th.ref_agent_light(st["shape"][:1], tables, 0, 1)
    assert decided, "a condition on the case: 1e-3 m clear of touching"
    assert int(out["agent_light"]) == want == bits
    if not present:
        assert not out["lights"].any() and not out["lights_mask"].any() and (out["lights_index"] == -1).all()
    else:
        me = st["shape"][0]
        for got, ref in zip((out["lights"], out["lights_mask"], out["lights_index"]),
                            th.ref_lights(tables, 0, me["cx"], me["cy"], me["c"], me["s"], 80.0, 8, 1)):
            assert got.tobytes() == ref.tobytes()


# -- 4. timing -----------------------------------------------------------------------------------------------------------------------
def test_a_light_acts_with_the_status_of_the_step_before_and_shows_this_step_s():
    status = [G, G, R, R, G]
    for t in range(9):
        out, _, _ = th.run_world([(0.0, 0.0, 0.0, status)], (0.0, 0.0, 0.0), clock=t)
        acting = 0 if t == 0 else 1 << (status[min(t - 1, 4)] - 1)
        assert int(out["agent_light"]) == acting, t
        assert out["lights"][0, 4] == status[min(t, 4)] and out["lights_mask"][0] == 1, t
    # the clock 0 .. 8: no flag, green, green, red, red, green and green from then on
    assert [int(th.run_world([(0.0, 0.0, 0.0, status)], (0.0, 0.0, 0.0), clock=t)[0]["agent_light"]) for t in range(9)] == \
        [0, 1, 1, 4, 4, 1, 1, 1, 1]


# -- 5. selection --------------------------------------------------------------------------------------------------------------------
def _select(lights, ego, cfg, clock=2):
    out, tables, st = th.run_world(lights, ego, clock=clock, cfg=cfg)
    me = st["shape"][0]
    c = dict(dict(num_lights=8, radius=80.0), **cfg)
    ref = th.ref_lights(tables, 0, me["cx"], me["cy"], me["c"], me["s"], c["radius"], c["num_lights"], clock)
    for got, want in zip((out["lights"], out["lights_mask"], out["lights_index"]), ref):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    return out


def test_two_lights_on_one_stop_point_order_by_ordinal():
    out = _select([(30.0, 1.0, 0.0, [R]), (12.0, -2.0, 0.3, [G]), (12.0, -2.0, 1.3, [Y]), (5.0, 0.0, 0.0, [U])], (1.0, 2.0, 0.4), dict(num_lights=4))
    assert out["lights_index"].tolist() == [3, 1, 2, 0] and out["lights"][1, 5] == out["lights"][2, 5]
    assert out["lights"][:, 4].tolist() == [U, G, Y, R]


def test_more_candidates_than_ranks_and_fewer():
    lights = [(3.0 * (7 - i), 0.5 * i, 0.1 * i, [G, R]) for i in range(7)]
    out = _select(lights, (0.0, 0.0, 0.0), dict(num_lights=3))
    assert out["lights_index"].tolist() == [6, 5, 4] and out["lights_mask"].tolist() == [1, 1, 1]
    out = _select(lights[:2], (0.0, 0.0, 0.0), dict(num_lights=5))
    assert out["lights_index"].tolist() == [1, 0, -1, -1, -1] and out["lights_mask"].tolist() == [1, 1, 0, 0, 0] and not out["lights"][2:].any()
    out = _select(lights, (0.0, 0.0, 0.0), dict(num_lights=0))
    assert out["lights"].shape == (0, 6) and int(out["agent_light"]) == 0


def test_a_light_exactly_on_the_radius_counts():
    out = _select([(80.0, 0.0, 0.0, [G]), (0.0, -80.0, 0.0, [R]), (80.25, 0.0, 0.0, [Y]), (60.0, 60.0, 0.0, [Y])], (0.0, 0.0, 0.0),
                  dict(num_lights=4, radius=80.0))
    assert out["lights_index"].tolist() == [0, 1, -1, -1] and out["lights"][:2, 5].tolist() == [6400.0, 6400.0]


# -- 6. config -----------------------------------------------------------------------------------------------------------------------
def test_defaults_and_checks():
    from metadrive_ped_amd.config import TRAFFIC_LIGHTS_DEFAULT_CONFIG, check_traffic_lights
    assert TRAFFIC_LIGHTS_DEFAULT_CONFIG == dict(num_lights=8, radius=80.0)
    cfg = make_scenario_config({})
    assert cfg["traffic_lights"] is None and cfg["skip_missing_light"] is True and cfg["no_light"] is False
    assert make_scenario_config(dict(traffic_lights={}))["traffic_lights"] == dict(num_lights=8, radius=80.0)
    assert make_scenario_config(dict(traffic_lights=dict(num_lights=3), skip_missing_light=False, no_light=False))["traffic_lights"]["num_lights"] == 3
    assert make_scenario_config(dict(no_light=True))["traffic_lights"] is None
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['colour'\]"):
        check_traffic_lights(dict(colour=1))
    for bad in (dict(num_lights=33), dict(num_lights=-1), dict(num_lights=2.0), dict(radius=0.0), dict(radius="far")):
        with pytest.raises(ValueError, match="traffic_lights\\['%s'\\]" % list(bad)[0]):
            make_scenario_config(dict(traffic_lights=bad))
    with pytest.raises(ValueError, match="None \\(off\\) or a dict"):
        make_scenario_config(dict(traffic_lights=True))


def test_no_light_with_the_key_names_both():
    with pytest.raises(ValueError) as err:
        make_scenario_config(dict(traffic_lights={}, no_light=True))
    assert "traffic_lights" in str(err.value) and "no_light=True" in str(err.value)


def test_the_keys_belong_to_the_scenario_envs():
    from metadrive_ped_amd.config import make_config
    for key, value in (("traffic_lights", {}), ("skip_missing_light", True)):
        with pytest.raises(KeyError, match=key):
            make_config({key: value})


def _env_with_a_stub_engine(cfg, agent_light):
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    env = BatchedScenarioEnv(dict(num_envs=2, num_scenarios=2, **cfg), scenarios=[synthetic_scenario(5, T=20, n_lights=1)] * 2)
    z = torch.zeros
    env.engine = SimpleNamespace(flags=z((2, 1), dtype=torch.int32), step_info=z((2, 1, 8)), nav_i=z((2, 1, 16), dtype=torch.int32), cost=z((2, 1)),
                                 action=z((2, 1, 2)), host=SimpleNamespace(walk=False),
                                 traffic_lights_out=None if agent_light is None else {"agent_light": torch.tensor(agent_light, dtype=torch.uint8)})
    return env


def test_default_off_leaves_the_env_without_the_info_keys():
    env = _env_with_a_stub_engine({}, None)
    info = env._info()
    assert not {"red_light", "yellow_light", "green_light"} & set(info)
    for call in (env.traffic_lights, env.traffic_lights_spec, lambda: env.traffic_light_ids(0)):
        with pytest.raises(RuntimeError, match="traffic_lights"):
            call()


def test_the_info_keys_and_the_spec_with_the_key():
    env = _env_with_a_stub_engine(dict(traffic_lights=dict(num_lights=3)), [4, 3])
    info = env._info()
    assert info["red_light"].tolist() == [True, False] and info["yellow_light"].tolist() == [False, True]
    assert info["green_light"].tolist() == [False, True] and str(info["red_light"].dtype) == "torch.bool"
    assert env.traffic_lights_spec() == {"agent_light": ((2, ), np.uint8), "lights": ((2, 3, 6), np.float32), "lights_mask": ((2, 3), np.uint8),
                                         "lights_index": ((2, 3), np.int32)}
