"""Crossing pedestrians (include/md_ped.h) on the host: known answers of the rule on hand-built states (tests/ped_host.c, the gcc
build of the header), the scene builder's placement, and the rule together with the CPU oracle -- md_ped applied to the oracle's
state before each of its steps, which is what tests/test_gpu_ped.py compares the device with."""
import math

import numpy as np
import pytest

import ped_host
from helpers import scripted_actions
from metadrive_ped_amd import abi

STEP_DT = 0.1                      # physics_world_step_size 0.02 x decision_repeat 5
A0, B0 = (3.0, 2.0), (3.0, 12.3)   # a crossing of L = 10.3 m, no multiple of the 0.12 m a step covers


def _ped(**kw):
    return abi.make_md_ped(dict(ped_host.DEFAULTS, **kw))


def _step(st, k, ped):
    ped_host.apply(st, k, ped)
    ped_host.walk(st, k)


def test_lone_pedestrian_walks_waits_and_returns():
    draws = (7, 3, 0, 0, 0, 0, 0, 0)
    st, k, ped = ped_host.blank_state(8), ped_host.config_struct(1, 8), _ped()
    ped_host.put_pedestrian(st, 5, A0, B0, draws=draws)
    want_steps = math.ceil(10.3 / (1.2 * STEP_DT))
    assert want_steps == 86

    def leg(phase, end):
        n = 0
        while True:
            _step(st, k, ped)
            if st["nav"]["toll_state"][5] != phase:
                break
            assert st["dyn"]["speed"][5] > 0 and n < 200
            n += 1
        assert n == want_steps
        assert math.hypot(st["shape"]["cx"][5] - end[0], st["shape"]["cy"][5] - end[1]) <= 1e-3
        return n

    def wait(phase):
        n = 1                                                  # the step that noticed the arrival stood as well
        assert st["dyn"]["speed"][5] == 0.0 and st["dyn"]["steering"][5] == 0.0 and st["dyn"]["throttle"][5] == 0.0
        while True:
            _step(st, k, ped)
            if st["nav"]["toll_state"][5] != phase:
                return n
            assert st["dyn"]["speed"][5] == 0.0
            n += 1

    leg(abi.PED_CROSS_AB, B0)
    assert st["nav"]["toll_state"][5] == abi.PED_WAIT_B and st["nav"]["timer"][5] == 10 + 7 and st["nav"]["rand_cursor"][5] == 1
    assert wait(abi.PED_WAIT_B) == 10 + 7
    # the step that ended the wait walked already: one step of the way back is done
    assert st["nav"]["toll_state"][5] == abi.PED_CROSS_BA and st["dyn"]["speed"][5] == np.float32(1.2)
    assert abs(st["dyn"]["heading"][5] - (-math.pi / 2)) < 1e-6 and abs(st["shape"]["s"][5] + 1.0) < 1e-6
    n = 1
    while st["nav"]["toll_state"][5] == abi.PED_CROSS_BA:
        _step(st, k, ped)
        n += 1
    assert n - 1 == want_steps
    assert math.hypot(st["shape"]["cx"][5] - A0[0], st["shape"]["cy"][5] - A0[1]) <= 1e-3
    assert st["nav"]["timer"][5] == 10 + 3 and st["nav"]["rand_cursor"][5] == 2
    assert wait(abi.PED_WAIT_A) == 10 + 3


def test_wait_draws_wrap_around_the_row():
    st, k, ped = ped_host.blank_state(4), ped_host.config_struct(1, 4), _ped(wait_min_steps=0)
    ped_host.put_pedestrian(st, 2, (0, 0), (0, 0.5), draws=(1, 2, 3, 4, 5, 6, 7, 8))
    seen = []
    for _ in range(400):
        before = int(st["nav"]["rand_cursor"][2])
        _step(st, k, ped)
        if st["nav"]["rand_cursor"][2] != before:
            seen.append(int(st["nav"]["timer"][2]))
    assert seen[:10] == [1, 2, 3, 4, 5, 6, 7, 8, 1, 2]


# a vehicle driving along +x towards the crossing x = 0 from x = -d, in the lane y = 5, at 10 m/s, half length 2.25:
# its arrival time is (d - 2.25) / 10
def _kerb_case(d, **veh):
    st, k = ped_host.blank_state(8), ped_host.config_struct(1, 8)
    ped_host.put_pedestrian(st, 6, (0, 0), (0, 10))
    ped_host.put_vehicle(st, 1, -d, 5.0, 0.0, 10.0, **veh)
    ped_host.apply(st, k, _ped())
    return st


def test_kerb_hold_threshold():
    t = 10.0 / 1.2 + 1.0                       # L / speed + time_margin
    d = 2.25 + 10.0 * t
    held = _kerb_case(d - 0.05)
    assert held["nav"]["toll_state"][6] == abi.PED_WAIT_A and held["dyn"]["speed"][6] == 0.0
    gone = _kerb_case(d + 0.05)
    assert gone["nav"]["toll_state"][6] == abi.PED_CROSS_AB and gone["dyn"]["throttle"][6] == np.float32(1.2)
    # the strip reaches `margin` beyond both kerbs, and no farther
    for y, want in ((-0.9, abi.PED_WAIT_A), (-1.1, abi.PED_CROSS_AB), (10.9, abi.PED_WAIT_A), (11.1, abi.PED_CROSS_AB)):
        st, k = ped_host.blank_state(8), ped_host.config_struct(1, 8)
        ped_host.put_pedestrian(st, 6, (0, 0), (0, 10))
        ped_host.put_vehicle(st, 1, -20.0, y, 0.0, 10.0)
        ped_host.apply(st, k, _ped())
        assert st["nav"]["toll_state"][6] == want, y
    # a standing vehicle holds the pedestrian only while it occupies the strip: |lon| <= hl + clear_dist
    for x, want in ((3.2, abi.PED_WAIT_A), (3.3, abi.PED_CROSS_AB)):
        st, k = ped_host.blank_state(8), ped_host.config_struct(1, 8)
        ped_host.put_pedestrian(st, 6, (0, 0), (0, 10))
        ped_host.put_vehicle(st, 1, x, 5.0, 0.0, 0.0)
        ped_host.apply(st, k, _ped())
        assert st["nav"]["toll_state"][6] == want, x


def test_countdown_comes_first():
    st, k = ped_host.blank_state(8), ped_host.config_struct(1, 8)
    ped_host.put_pedestrian(st, 6, (0, 0), (0, 10), countdown=3)
    for left in (2, 1):
        ped_host.apply(st, k, _ped())
        assert st["nav"]["timer"][6] == left and st["nav"]["toll_state"][6] == abi.PED_WAIT_A
    ped_host.apply(st, k, _ped())
    assert st["nav"]["timer"][6] == 0 and st["nav"]["toll_state"][6] == abi.PED_CROSS_AB


def _crossing_case(d, veh_y=4.0, phase=abi.PED_CROSS_AB, at=(0.0, 2.0), **veh):
    st, k = ped_host.blank_state(8), ped_host.config_struct(1, 8)
    ped_host.put_pedestrian(st, 6, (0, 0), (0, 10), phase=phase, at=at)
    ped_host.put_vehicle(st, 1, -d, veh_y, 0.0, 10.0, **veh)
    ped_host.apply(st, k, _ped())
    return st


def test_mid_crossing_stop_threshold():
    d = 2.25 + 10.0 * 1.5                      # yield_time
    stop = _crossing_case(d - 0.05)
    assert stop["nav"]["toll_state"][6] == abi.PED_CROSS_AB and stop["dyn"]["speed"][6] == 0.0 and stop["dyn"]["throttle"][6] == 0.0
    go = _crossing_case(d + 0.05)
    assert go["dyn"]["speed"][6] == np.float32(1.2) and go["dyn"]["throttle"][6] == np.float32(1.2) and go["dyn"]["steering"][6] == 0.0
    # ahead means within yield_ahead metres of the pedestrian in ITS walking direction
    assert _crossing_case(d - 0.05, veh_y=4.9)["dyn"]["speed"][6] == 0.0
    assert _crossing_case(d - 0.05, veh_y=5.1)["dyn"]["speed"][6] == np.float32(1.2)
    assert _crossing_case(d - 0.05, veh_y=1.9)["dyn"]["speed"][6] == np.float32(1.2)          # behind its back
    back = _crossing_case(d - 0.05, veh_y=1.0, phase=abi.PED_CROSS_BA)                          # walking B -> A: y = 1 lies ahead
    assert back["dyn"]["speed"][6] == 0.0
    assert _crossing_case(d - 0.05, veh_y=4.0, phase=abi.PED_CROSS_BA)["dyn"]["throttle"][6] == np.float32(-1.2)


def test_vehicles_that_never_count():
    near = 20.0                                # arrival in 1.8 s: holds at the kerb and stops a crossing when it counts
    assert _kerb_case(near)["nav"]["toll_state"][6] == abi.PED_WAIT_A
    assert _crossing_case(near - 5)["dyn"]["speed"][6] == 0.0
    for flags in (abi.F_ALIVE | abi.F_PENDING, abi.F_ALIVE | abi.F_STATIC, 0):
        assert _kerb_case(near, flags=flags)["nav"]["toll_state"][6] == abi.PED_CROSS_AB, flags
        assert _crossing_case(near - 5, flags=flags)["dyn"]["speed"][6] == np.float32(1.2), flags
    # moving away: the same distance on the far side of the crossing line
    assert _kerb_case(-near)["nav"]["toll_state"][6] == abi.PED_CROSS_AB
    assert _crossing_case(-(near - 5))["dyn"]["speed"][6] == np.float32(1.2)
    # another pedestrian and a cone on the line do not count either
    st, k = ped_host.blank_state(8), ped_host.config_struct(1, 8)
    ped_host.put_pedestrian(st, 6, (0, 0), (0, 10))
    ped_host.put_pedestrian(st, 5, (0, 0), (0, 10), phase=abi.PED_CROSS_AB, at=(0.0, 1.0))
    st["shape"][4] = st["shape"][5]
    st["shape"]["flags"][4] = abi.KIND_CONE | abi.F_ALIVE | abi.F_STATIC
    ped_host.apply(st, k, _ped())
    assert st["nav"]["toll_state"][6] == abi.PED_CROSS_AB


def test_user_spawned_participant_is_left_alone():
    from metadrive_ped_amd import participants as P
    st, k = ped_host.blank_state(8), ped_host.config_struct(1, 8)
    st["shape0"], st["flags"] = st["shape"].copy(), np.zeros(8, np.uint32)
    ped_host.put_vehicle(st, 1, -10.0, 0.0, 0.0, 10.0)
    slot = P.spawn(st, 1, 8, 1, "pedestrian", [0.0, 3.0], heading_theta=0.3)
    P.set_velocity(st, 1, 8, slot, [1, 0], 1.4, in_local_frame=True)
    cyc = P.spawn(st, 1, 8, 1, "cyclist", [5.0, 3.0])
    st["nav"]["toll_state"][cyc] = abi.PED_WAIT_A          # a cyclist is no pedestrian, whatever its row holds
    before = {k_: v.copy() for k_, v in st.items()}
    ped_host.apply(st, k, _ped())
    for k_ in st:
        assert st[k_].tobytes() == before[k_].tobytes(), k_


def test_env_about_to_reset_is_skipped():
    st, k = ped_host.blank_state(8, E=2), ped_host.config_struct(2, 8)
    for e in (0, 1):
        ped_host.put_pedestrian(st, e * 8 + 6, (0, 0), (0, 10))
    st["need_reset"][0] = 1
    ped_host.apply(st, k, _ped())
    assert st["nav"]["toll_state"][6] == abi.PED_WAIT_A and st["nav"]["toll_state"][14] == abi.PED_CROSS_AB


# ---- scene building -------------------------------------------------------------------------------------------------------------
PG = dict(num_envs=8, num_scenarios=8, map="SCX", traffic_density=0.15, horizon=30, build_workers=1)


def _host(**kw):
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    return HostScene(make_config(dict(PG, **kw)))


@pytest.fixture(scope="module")
def host3():
    return _host(num_pedestrians=3, mover_capacity=32)


def test_scenes_are_deterministic_per_seed(host3):
    again = _host(num_pedestrians=3, mover_capacity=32)
    for k, v in host3.state.items():
        assert v.tobytes() == again.state[k].tobytes(), k
    assert [sc.ped_slots for sc in host3.scenes.values()] == [[31, 30, 29]] * 8       # from the top down, like props


def test_everything_but_the_pedestrians_is_the_scene_without_them(host3):
    plain = _host(mover_capacity=32)
    peds = ped_host.driven_slots(host3.state, 8, 32).reshape(-1)
    assert peds.sum() == 24 and not ped_host.driven_slots(plain.state, 8, 32).any()
    for k, v in host3.state.items():
        a, b = v.view(np.uint8).reshape(len(v), -1), plain.state[k].view(np.uint8).reshape(len(v), -1)
        if len(v) == 8 * 32:
            assert np.array_equal(a[~peds], b[~peds]), k
            if k in ("shape", "shape0", "pid", "pid0", "nav", "nav0"):
                assert not np.array_equal(a[peds], b[peds]), k
        else:
            assert np.array_equal(a, b), k
    for k, v in host3.world.arrays.items():
        assert v.tobytes() == plain.world.arrays[k].tobytes(), k
    # the auto capacity counts them
    assert _host(num_pedestrians=3).cap >= _host().cap


def test_live_and_snapshot_rows_agree(host3):
    for k in ("shape", "dyn", "nav", "pid"):
        assert host3.state[k].tobytes() == host3.state[k + "0"].tobytes(), k


def test_sites_lie_off_the_lanes_and_cross_the_road(host3):
    """`Off every lane`: for every lane of the map the end point lies outside the lane's own extent -- |lateral| > width / 2
    wherever its station falls inside [0, length] (the lateral coordinate against a lane's endless centre line says nothing about
    a point beside another road)."""
    from metadrive_ped_amd.mapgen.pg import negate_road
    for seed, sc in host3.scenes.items():
        net = sc.tables.pg_map.net
        assert len(sc.ped_sites) == 3
        for slot, ((a, b), s) in zip(sc.ped_slots, sc.ped_sites):
            p = sc.pid[slot]
            A, B = np.array([p["hp"], p["hi"]], np.float64), np.array([p["hd"], p["lp"]], np.float64)
            for _, _, lanes in net.roads():
                for l in lanes:
                    for q in (A, B):
                        st, lat = l.local_coordinates(q)
                        assert not (0 <= st <= l.length) or abs(lat) > l.width / 2, (seed, slot, l.index)
            lanes = list(net.lanes(a, b))
            ra, rb = negate_road(a, b)
            if ra in net.graph and rb in net.graph[ra]:
                lanes += list(net.lanes(ra, rb))
            ab = B - A
            L = math.hypot(*ab)
            for l in lanes:
                # perpendicular: the end points are float32 at up to a few hundred metres (ulp ~3e-5 m), L >= 5 m
                assert abs(float(np.dot(ab, l.direction))) / L < 1e-4, (seed, slot)
                (sa, la), (sb, lb) = l.local_coordinates(A), l.local_coordinates(B)
                assert 0 < sa < l.length and 0 < sb < l.length
                assert la * lb < 0 and abs(la) > l.width / 2 and abs(lb) > l.width / 2, (seed, slot, l.index)
            assert abs(float(p["ld"]) - math.atan2(ab[1], ab[0])) < 1e-6
            # the walker stands on one of the two end points, waiting
            pos = np.array([sc.shape[slot]["cx"], sc.shape[slot]["cy"]], np.float64)
            at_b = sc.nav[slot]["toll_state"] == abi.PED_WAIT_B
            assert sc.nav[slot]["toll_state"] in (abi.PED_WAIT_A, abi.PED_WAIT_B) and np.array_equal(pos, B if at_b else A)
            assert 0 <= sc.nav[slot]["timer"] < 25 and ((0 <= sc.idm_rand[slot]) & (sc.idm_rand[slot] < 25)).all()
            agent = np.array([sc.shape[0]["cx"], sc.shape[0]["cy"]], np.float64)
            t = min(1.0, max(0.0, float(np.dot(agent - A, ab)) / (L * L)))
            assert math.hypot(*(A + t * ab - agent)) >= 15.0


def test_props_keep_their_slots_above_the_pedestrians():
    """SafeMetaDriveEnv's accident scenes: cones, barriers and broken-down vehicles fill the slots from the top down, the
    pedestrians follow below them, and the scene's other rows are those of the scene without pedestrians"""
    safe = dict(accident_prob=0.8, traffic_density=0.05, crash_vehicle_done=False, crash_object_done=False, mover_capacity=64)
    host, plain = _host(num_pedestrians=2, **safe), _host(**safe)
    peds = ped_host.driven_slots(host.state, 8, 64)
    props = ((plain.state["shape0"]["flags"] & abi.F_STATIC) != 0).reshape(8, 64)
    assert props.sum() >= 8 and (peds.sum(axis=1) == 2).all()
    for e in range(8):
        lowest_prop = np.nonzero(props[e])[0].min() if props[e].any() else 64
        assert np.nonzero(peds[e])[0].tolist() == [lowest_prop - 2, lowest_prop - 1]
    for k, v in host.state.items():
        if len(v) == 8 * 64:
            rows = ~peds.reshape(-1)
            assert v[rows].tobytes() == plain.state[k][rows].tobytes(), k


def test_a_map_without_a_straight_road_holds_none():
    host = _host(num_pedestrians=2, pedestrian_config=dict(min_road_length=5000.0))
    assert not ped_host.driven_slots(host.state, 8, host.cap).any()
    assert [sc.ped_slots for sc in host.scenes.values()] == [[]] * 8


def test_refusals_by_name():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.scenario import make_scenario_config
    with pytest.raises(NotImplementedError, match="multi-agent"):
        make_config(dict(is_multi_agent=True, marl_map="roundabout", num_agents=4, traffic_density=0.0, num_pedestrians=1))
    with pytest.raises(NotImplementedError, match="replay"):
        make_config(dict(traffic_mode="replay", num_pedestrians=1))
    with pytest.raises(NotImplementedError, match="BatchedScenarioEnv"):
        make_scenario_config(dict(num_pedestrians=1))
    with pytest.raises(KeyError):
        make_config(dict(num_pedestrians=1, pedestrian_config=dict(pace=1.0)))
    with pytest.raises(ValueError, match="speed"):
        make_config(dict(num_pedestrians=1, pedestrian_config=dict(speed=0.0)))
    assert make_config({})["num_pedestrians"] == 0


# ---- with the oracle ------------------------------------------------------------------------------------------------------------
def test_auto_reset_restores_the_pedestrians(host3):
    import oracle_binding as ob
    orc, ped = ob.OracleWorld(host3), abi.make_md_ped(host3.cfg["pedestrian_config"])
    orc.reset()
    peds = ped_host.driven_slots(host3.state, 8, 32).reshape(-1)
    restored = 0
    for t in range(45):
        ped_host.apply(orc.state, orc.k, ped)
        resetting = np.repeat(orc.state["need_reset"] != 0, 32)
        orc.step(scripted_actions(8, 1, t))
        rows = peds & resetting
        for k in ("shape", "dyn", "nav", "pid"):
            assert orc.state[k][rows].tobytes() == orc.state[k + "0"][rows].tobytes(), (t, k)
        moved = peds & ~resetting
        restored += int(rows.sum())
        if t > 27:
            assert orc.state["nav"][moved].tobytes() != orc.state["nav0"][moved].tobytes()
    assert restored >= 3 * 8      # horizon 30: every env has reset itself once


def test_idm_agent_rollout_reaches_every_phase():
    """Two lanes a side (a 16 m crossing, 134 steps) so that a walker gets across and back within the run"""
    host = _host(num_envs=2, num_scenarios=2, num_pedestrians=3, agent_policy="IDMPolicy", horizon=1000, traffic_density=0.1,
                 map_config=dict(lane_num=2))
    cover = ped_host.Coverage()
    first = {}

    def each(t, orc):
        ph = orc.state["nav"]["toll_state"].reshape(2, host.cap)
        for e, j in zip(*np.nonzero(ped_host.driven_slots(orc.state, 2, host.cap))):
            first.setdefault((e, j), []).append(int(ph[e, j]))

    ped_host.rollout(host, 240, lambda t: None, cover=cover, each=each)
    assert cover.phases == {1, 2, 3, 4} and cover.arrivals >= 1
    # one walker went through a whole cycle: wait, cross, wait at the other end, cross back
    cycles = [[p for i, p in enumerate(seq) if i == 0 or p != seq[i - 1]] for seq in first.values()]
    assert any(len(c) >= 4 for c in cycles), cycles


# (start seed, config) of the parity runs of tests/test_gpu_ped.py: the start seeds at which the host alone (the rule + the oracle)
# shows a kerb hold AND a mid-crossing stop within 60 scripted steps, found with this very rollout
PARITY_RUNS = dict(
    default=(19, dict()),
    respawn=(19, dict(traffic_mode="respawn")),                      # the RESPAWN kernel variant
    wave=(180, dict(step_kernel="wave", num_scenarios=1)),           # the wave kernel, one shared map
    cap96=(19, dict(mover_capacity=96)),                             # two lane rounds
    envs5=(179, dict(num_envs=5)),                                   # the last block of md_ped is not full
    one=(436, dict(num_pedestrians=1)),
)


@pytest.mark.parametrize("name", list(PARITY_RUNS))
def test_traffic_holds_and_stops_pedestrians(name):
    seed, extra = PARITY_RUNS[name]
    host = _host(**dict(dict(num_pedestrians=3, start_seed=seed), **extra))
    cover, resets = ped_host.Coverage(), np.zeros(host.E, np.int64)

    def each(t, orc):
        resets[:] += orc.state["need_reset"] != 0

    ped_host.rollout(host, 60, lambda t: scripted_actions(host.E, 1, t), cover=cover, each=each)
    assert cover.kerb_holds >= 1 and cover.mid_stops >= 1 and (resets >= 1).all()
