"""The vector scene observation (include/md_vector_obs.h) on the CPU, through its gcc host build (tests/vector_obs_host.py): known
answers on hand-built states with exactly representable numbers, the history ring with frames pushed by hand, the route against a
float64 restatement, invariants over oracle rollouts, and the config / env API that needs no device."""
import math

import numpy as np
import pytest

import vector_obs_host as vh
from helpers import scripted_actions
from metadrive_ped_amd import abi
from metadrive_ped_amd.config import VECTOR_OBS_DEFAULT_CONFIG, VECTOR_OBS_RANGES, make_config

# Route: the largest distance between a host-build waypoint (float32) and its float64 restatement measured here on the "SC" map is
# 2.72e-5 m (test_route_against_float64 prints it); the bound asserted everywhere is four times that, because other maps have
# larger coordinates.  The sanity cap is a centimetre.
ROUTE_MEASURED = 2.72e-5
ROUTE_BOUND = 4 * ROUTE_MEASURED
assert ROUTE_BOUND < 1e-2


def _run(cfg, st_edit=None, cap=8, **world):
    w, s, k, st, tables = vh.straight_world(cap=cap, **world)
    if st_edit:
        st_edit(st)
    hv = vh.HostVectorObs(dict(vh.SMALL, **cfg), 1, 1, cap)
    hv.run(w, s, k)
    return hv.outputs(), hv, (w, s, k, st, tables)


# -- 1. neighbours: known answers ------------------------------------------------------------------------------------------------
def test_neighbours_come_out_nearest_first_in_the_ego_frame():
    def edit(st):
        vh.put(st, 1, -6.0, 8.0, speed=3.0, kind=abi.KIND_CYCLIST, hl=0.5, hw=0.25)
        vh.put(st, 2, 3.0, 4.0, math.pi / 2, hl=2.25, hw=0.75)
    o, _, _ = _run({}, edit)
    a, m = o["agents"][0, 0], o["agents_mask"][0, 0]
    assert a[0, 0].tolist()[:2] == [3.0, 4.0] and a[1, 0].tolist()[:2] == [-6.0, 8.0]
    assert abs(a[0, 0, 2]) < 1e-7 and a[0, 0, 3] == 1.0 and a[1, 0, 2:].tolist() == [1.0, 0.0]
    assert m.tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 0]] and not a[2].any() and not a[:, 1:].any()
    assert o["agents_meta"][0, 0].tolist() == [[4.5, 1.5, 0.0, float(abi.KIND_VEHICLE)], [1.0, 0.5, 3.0, float(abi.KIND_CYCLIST)], [0.0] * 4]
    assert o["ego"][0, 0].tolist() == [[0.0, 0.0, 1.0, 0.0], [0.0] * 4, [0.0] * 4] and o["ego_mask"][0, 0].tolist() == [1, 0, 0]


def test_the_ego_frame_turns_with_the_observer():
    def edit(st):
        vh.put(st, 0, 10.0, 0.0, math.pi / 2, flags=abi.F_ALIVE | abi.F_AGENT)      # looks along +y
        vh.put(st, 1, 10.0, 5.0)                                                    # 5 m ahead, heading -90 deg in the ego frame
        vh.put(st, 2, 7.0, 0.0)                                                     # 3 m to the left
    o, _, _ = _run({}, edit)
    a = o["agents"][0, 0, :, 0]
    assert np.allclose(a[0], [0.0, 3.0, 0.0, -1.0], atol=1e-6) and np.allclose(a[1], [5.0, 0.0, 0.0, -1.0], atol=1e-6)


def test_equal_distances_come_out_in_slot_order():
    def edit(st):
        vh.put(st, 5, 0.0, 5.0)
        vh.put(st, 2, 5.0, 0.0)
        vh.put(st, 3, -3.0, 4.0)
    o, _, _ = _run({}, edit)
    assert o["agents"][0, 0, :, 0, :2].tolist() == [[5.0, 0.0], [-3.0, 4.0], [0.0, 5.0]]


def test_the_radius_is_inclusive_and_squared():
    def edit(st):
        vh.put(st, 1, 30.0, 40.0)                                        # d2 = 2500 = radius^2: kept
        vh.put(st, 2, 30.0, 40.0078125)                                  # d2 = 2500.625...: just outside, dropped
        vh.put(st, 3, 0.0, -50.0, kind=abi.KIND_CONE, flags=abi.F_ALIVE | abi.F_STATIC)  # a prop counts
        vh.put(st, 4, 1.0, 1.0, flags=0)                                 # not alive: no candidate
    o, _, _ = _run(dict(radius=50.0), edit)
    assert o["agents_mask"][0, 0, :, 0].tolist() == [1, 1, 0]
    assert o["agents"][0, 0, :2, 0, :2].tolist() == [[30.0, 40.0], [0.0, -50.0]]
    assert o["agents_meta"][0, 0, 1, 3] == float(abi.KIND_CONE)


def test_only_the_nearest_k_appear():
    def edit(st):
        for j, x in enumerate((9.0, 2.0, 7.0, 4.0, 6.0), start=1):
            vh.put(st, j, x, 0.0)
    o, _, _ = _run(dict(num_agents=3), edit)
    assert o["agents"][0, 0, :, 0, 0].tolist() == [2.0, 4.0, 6.0] and o["agents_mask"][0, 0, :, 0].tolist() == [1, 1, 1]
    one, _, _ = _run(dict(num_agents=1), edit)
    assert one["agents"].shape == (1, 1, 1, 3, 4) and one["agents"][0, 0, 0, 0, 0] == 2.0


def test_an_invalid_observer_is_all_zero():
    def off_lane(st):
        vh.put(st, 1, 3.0, 4.0)
        st["nav"]["lane"][0] = -1
    def static(st):
        vh.put(st, 1, 3.0, 4.0)
        st["shape"]["flags"][0] |= abi.F_STATIC
    for edit in (off_lane, static):
        o, hv, _ = _run({}, edit)
        assert all(not v.any() for v in o.values())
        assert hv.history()["cursor"][0].tolist() == [0, 1, 0, 0]       # the frame is pushed all the same


# -- 2. history: frames pushed by hand ---------------------------------------------------------------------------------------------
def _frames(frames, cfg=None, cap=8):
    """frames: one edit(st) per call, the last through the whole rule; the clock (MdNav.steps of slot 0) counts up from 1"""
    w, s, k, st, _ = vh.straight_world(cap=cap)
    hv = vh.HostVectorObs(dict(vh.SMALL, **(cfg or {})), 1, 1, cap)
    for t, edit in enumerate(frames):
        st["nav"]["steps"][0] = t + 1
        edit(st)
        (hv.run(w, s, k) if t == len(frames) - 1 else hv.push(s, k))
    return hv.outputs(), hv


def test_history_rows_are_in_the_current_ego_frame():
    def at(x_ego, x_other):
        def edit(st):
            vh.put(st, 0, x_ego, 0.0, flags=abi.F_ALIVE | abi.F_AGENT)
            vh.put(st, 1, x_other, 2.0)
        return edit
    o, hv = _frames([at(0.0, 10.0), at(1.0, 12.0), at(2.0, 14.0)])
    assert o["ego"][0, 0].tolist() == [[0.0, 0.0, 1.0, 0.0], [-1.0, 0.0, 1.0, 0.0], [-2.0, 0.0, 1.0, 0.0]]
    assert o["agents"][0, 0, 0].tolist() == [[12.0, 2.0, 1.0, 0.0], [10.0, 2.0, 1.0, 0.0], [8.0, 2.0, 1.0, 0.0]]
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 1, 1] and o["ego_mask"][0, 0].tolist() == [1, 1, 1]
    assert hv.history()["cursor"][0].tolist() == [2, 3, 3, 0]
    # a fourth frame overwrites the oldest ring slot
    o, hv = _frames([at(0.0, 10.0), at(1.0, 12.0), at(2.0, 14.0), at(3.0, 16.0)])
    assert o["agents"][0, 0, 0, :, 0].tolist() == [13.0, 11.0, 9.0] and hv.history()["cursor"][0].tolist() == [0, 3, 4, 0]


def test_a_slot_absent_in_a_middle_frame_has_its_older_frames_masked():
    here = lambda st: vh.put(st, 1, 5.0, 0.0)
    gone = lambda st: vh.clear(st, 1)
    o, _ = _frames([here, gone, here])
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 0, 0] and not o["agents"][0, 0, 0, 1:].any()
    o, _ = _frames([gone, here, here])
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 1, 0]


def test_max_jump_is_inclusive_and_ends_the_history():
    at = lambda x: (lambda st: vh.put(st, 1, x, 0.0))
    o, _ = _frames([at(2.0), at(10.0), at(18.0)], dict(max_jump=8.0))
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 1, 1]
    above = float(np.nextafter(np.float32(18.0), np.float32(19.0)))
    o, _ = _frames([at(2.0), at(10.0), at(above)], dict(max_jump=8.0))
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 0, 0]
    o, _ = _frames([at(1.0), at(10.0), at(18.0)], dict(max_jump=8.0))     # the older link breaks, the newer one holds
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 1, 0]


def test_a_changed_kind_masks_the_older_frames():
    car = lambda st: vh.put(st, 1, 5.0, 0.0)
    bike = lambda st: vh.put(st, 1, 5.0, 0.0, kind=abi.KIND_CYCLIST)
    o, _ = _frames([car, car, bike])
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 0, 0]
    o, _ = _frames([bike, car, car])
    assert o["agents_mask"][0, 0, 0].tolist() == [1, 1, 0]


def test_the_clock_empties_the_ring():
    w, s, k, st, _ = vh.straight_world()
    vh.put(st, 1, 5.0, 0.0)
    hv = vh.HostVectorObs(dict(vh.SMALL), 1, 1, 8)
    for clock, held in ((5, 1), (6, 2), (7, 3), (8, 3), (3, 1), (4, 2), (0, 1), (0, 1), (1, 2)):
        st["nav"]["steps"][0] = clock
        hv.run(w, s, k)
        assert hv.history()["cursor"][0, 1:3].tolist() == [held, clock], (clock, held)
        assert hv.out("agents_mask")[0, 0, 0].tolist() == [1] * held + [0] * (3 - held)
        assert hv.out("ego_mask")[0, 0].tolist() == [1] * held + [0] * (3 - held)


def test_a_multi_agent_batch_reads_the_env_clock():
    w, s, k, st, _ = vh.straight_world(multi=True)
    hv = vh.HostVectorObs(dict(vh.SMALL), 1, 1, 8)
    st["nav"]["steps"][0] = 0           # a respawned agent's own counter: not the clock
    for clock, held in ((4, 1), (5, 2), (0, 1)):
        st["env_steps"][0] = clock
        hv.run(w, s, k)
        assert hv.history()["cursor"][0, 1:3].tolist() == [held, clock]


# -- 3. lanes and route on hand-built lanes ------------------------------------------------------------------------------------------
def test_lanes_nearest_first_sampled_end_to_end():
    o, _, _ = _run(dict(num_lanes=3, lane_points=3), n_lanes=2, length=200.0, width=3.5)
    assert o["lanes_mask"][0, 0].tolist() == [1, 1, 0]
    assert o["lanes"][0, 0, 0].tolist() == [[0.0, 0.0], [100.0, 0.0], [200.0, 0.0]]
    assert o["lanes"][0, 0, 1].tolist() == [[0.0, -3.5], [100.0, -3.5], [200.0, -3.5]] and not o["lanes"][0, 0, 2].any()
    assert o["lanes_meta"][0, 0].tolist() == [[3.5, 200.0, 1.0, 0.0], [3.5, 200.0, 1.0, 3.5], [0.0] * 4]


def test_waypoints_past_the_route_s_end_are_masked():
    o, _, _ = _run(dict(route_points=5, route_spacing=4.0), lambda st: vh.put(st, 0, 186.0, 0.0, flags=abi.F_ALIVE | abi.F_AGENT), length=200.0)
    assert o["route_mask"][0, 0].tolist() == [1, 1, 1, 0, 0]        # 190, 194, 198 lie on the lane; 202 and 206 do not
    assert o["route"][0, 0].tolist() == [[4.0, 0.0, 1.0, 0.0], [8.0, 0.0, 1.0, 0.0], [12.0, 0.0, 1.0, 0.0], [0.0] * 4, [0.0] * 4]
    o, _, _ = _run(dict(route_points=0, num_lanes=0))
    assert o["route"].shape == (1, 1, 0, 4) and o["lanes"].shape == (1, 1, 0, 3, 2) and o["agents_mask"][0, 0, 0, 0] == 0


# -- 4. the route against float64, on a generated map ------------------------------------------------------------------------------
def _chain(host, state, e, a):
    """(lane records of the chain, the chain's road ids) of observer a of env e, restated in numpy"""
    arr = host.world.arrays
    m = int(arr["env_map"][e])
    lanes = arr["lanes"][int(arr["lane_off"][m]):int(arr["lane_off"][m + 1])]
    roads = arr["roads"][int(arr["road_off"][m]):int(arr["road_off"][m + 1])]
    n = e * host.cap + a
    nav = state["nav"][n]
    cur = lanes[int(nav["lane"])]
    i_ref = int(cur["idx"]) if int(cur["road"]) == int(nav["road0"]) else 0
    rr = state["route_roads"].reshape(-1, abi.MD_ROUTE_LEN)[n]
    ids = []
    for i in range(int(nav["ck0"]), int(nav["route_len"]) - 1):
        if rr[i] < 0:
            break
        ids.append(int(rr[i]))
    return [lanes[int(roads[r]["first_lane"]) + min(i_ref, int(roads[r]["n_lanes"]) - 1)] for r in ids], ids, lanes


def _valid(state, n):
    f = int(state["shape"]["flags"][n])
    drives = (f & abi.F_ALIVE) and (f & abi.KIND_MASK) == abi.KIND_VEHICLE and not (f & (abi.F_STATIC | abi.F_PENDING))
    return bool(drives) and int(state["nav"]["lane"][n]) >= 0


def _position64(L, s):
    if int(L["type"]) == 0:
        return float(L["ax"]) + s * float(L["bx"]), float(L["ay"]) + s * float(L["by"]), float(L["heading"])
    phi = float(L["dirsign"]) * s / float(L["bx"]) + float(L["by"])
    return (float(L["ax"]) + float(L["bx"]) * math.cos(phi), float(L["ay"]) + float(L["bx"]) * math.sin(phi),
            phi + math.pi / 2 * float(L["dirsign"]))


def _route64(host, state, e, a, M, spacing):
    """-> rows [M, 4] float64, mask [M], lane type per waypoint (-1 masked): the header's route rule in float64"""
    chain, _, _ = _chain(host, state, e, a)
    sh = state["shape"][e * host.cap + a]
    cx, cy, c, s = (float(sh[k]) for k in ("cx", "cy", "c", "s"))
    rows, mask, kinds = np.zeros((M, 4)), np.zeros(M, np.uint8), np.full(M, -1)
    if not chain:
        return rows, mask, kinds
    s0 = min(max(vh.lane_local(chain[0], cx, cy)[0], 0.0), float(chain[0]["length"]))
    cum = [-s0]
    for L in chain:
        cum.append(cum[-1] + float(L["length"]))
    for p in range(M):
        d = (p + 1) * spacing
        for i, L in enumerate(chain):
            if d <= cum[i + 1]:
                x, y, h = _position64(L, d - cum[i])
                rx, ry, hc, hs = x - cx, y - cy, math.cos(h), math.sin(h)
                rows[p] = [rx * c + ry * s, ry * c - rx * s, hc * c + hs * s, hs * c - hc * s]
                mask[p], kinds[p] = 1, int(L["type"])
                break
    return rows, mask, kinds


def _pg_host(**kw):
    from metadrive_ped_amd.engine import HostScene
    return HostScene(make_config(dict(dict(num_envs=4, num_scenarios=4, map="CXO", traffic_density=0.3, agent_policy="IDMPolicy"), **kw)))


def test_route_against_float64():
    """Measured here: the largest |host build - float64| over the waypoints' coordinates is 2.72e-5 m (ROUTE_MEASURED; 32 waypoints 8 m
    apart over 60 IDM-driven steps on two "SC" maps); the bound asserted is four times that, 1.09e-4 m."""
    import oracle_binding as ob
    host = _pg_host(num_envs=2, num_scenarios=2, map="SC", traffic_density=0.0)
    orc = ob.OracleWorld(host)
    orc.reset()
    M, spacing = 32, 8.0
    hv = vh.HostVectorObs(dict(vh.SMALL, route_points=M, route_spacing=spacing), host.E, 1, host.cap)
    worst, on_circle, masked = 0.0, 0, 0
    for t in range(60):
        orc.step(None)
        hv.run(orc.w, orc.s, orc.k)
        for e in range(host.E):
            if not _valid(orc.state, e * host.cap):
                continue
            rows, mask, kinds = _route64(host, orc.state, e, 0, M, spacing)
            got, got_mask = hv.out("route")[e, 0], hv.out("route_mask")[e, 0]
            assert got_mask.tolist() == mask.tolist(), (t, e)
            worst = max(worst, float(np.abs(got[:, :2] - rows[:, :2]).max()))
            assert np.abs(got[:, 2:] - rows[:, 2:]).max() < 1e-5
            on_circle += int((kinds == 1).sum())
            masked += int((mask == 0).sum())
    print("route: largest |float32 - float64| = %.3g m" % worst)
    assert on_circle > 0 and masked > 0, "the run must put waypoints on the circular lane and past the route's end"
    assert worst <= ROUTE_BOUND


# -- 5. invariants over oracle rollouts ----------------------------------------------------------------------------------------------
class Seen:
    def __init__(self):
        self.enters = self.leaves = self.onto_circle = self.resets = self.invalid = self.observers = 0


def _check_invariants(host, state, hv, vo, prev, seen):
    """One step's outputs against the state they were computed from; `prev`: what the previous step left for the event counters"""
    E, A, cap = host.E, host.A, host.cap
    o = hv.outputs()
    clock = hv.history()["cursor"][:, 2]
    sh = state["shape"].reshape(E, cap)
    now = {}
    for e in range(E):
        reset = prev is not None and clock[e] <= prev["clock"][e]
        seen.resets += int(reset)
        for a in range(A):
            blocks = {k: v[e, a] for k, v in o.items()}
            seen.observers += 1
            if not _valid(state, e * cap + a):
                seen.invalid += 1
                assert all(not v.any() for v in blocks.values()), (e, a)
                continue
            me = sh[e, a]
            # neighbours ascend in d2
            n = int(blocks["agents_mask"][:, 0].sum())
            assert blocks["agents_mask"][:n, 0].all() and not blocks["agents_mask"][n:].any()
            d2 = (blocks["agents"][:n, 0, :2].astype(np.float64) ** 2).sum(axis=1)
            assert (np.diff(d2) >= -1e-3).all() and (d2 <= vo["radius"] ** 2 * (1 + 1e-5)).all(), (e, a, d2)
            present = ((sh[e]["flags"] & abi.F_ALIVE) != 0) & ((sh[e]["flags"] & abi.KIND_MASK) != 0)
            dist2 = (sh[e]["cx"].astype(np.float64) - float(me["cx"])) ** 2 + (sh[e]["cy"].astype(np.float64) - float(me["cy"])) ** 2
            inside = present & (dist2 <= vo["radius"] ** 2)
            inside[a] = False
            assert n == min(vo["num_agents"], int(inside.sum())), (e, a)
            now[(e, a)] = (present.copy(), inside.copy())
            if prev is not None and not reset and (e, a) in prev["near"]:
                was_present, was_inside = prev["near"][(e, a)]
                both = present & was_present
                both[a] = False
                seen.enters += int((both & inside & ~was_inside).sum())
                seen.leaves += int((both & ~inside & was_inside).sum())
            # waypoints lie on a lane of the chain
            chain, road_ids, lanes = _chain(host, state, e, a)
            _, mask64, kinds = _route64(host, state, e, a, vo["route_points"], vo["route_spacing"])
            assert blocks["route_mask"].tolist() == mask64.tolist()
            c, s = float(me["c"]), float(me["s"])
            for p in np.nonzero(blocks["route_mask"])[0]:
                x, y = (float(v) for v in blocks["route"][p, :2])
                wx, wy = float(me["cx"]) + x * c - y * s, float(me["cy"]) + x * s + y * c
                lat = min(abs(vh.lane_local(L, wx, wy)[1]) for L in chain)
                assert lat <= ROUTE_BOUND, (e, a, p, lat)
            if prev is not None and not reset and (e, a) in prev["kinds"]:
                seen.onto_circle += int(((prev["kinds"][(e, a)] == 0) & (kinds == 1)).sum())
            now[("kinds", e, a)] = kinds
            # lanes ascend in distance; on_route is the set test
            P = int(blocks["lanes_mask"].sum())
            assert P == min(vo["num_lanes"], len(lanes)) and blocks["lanes_mask"][:P].all()
            assert (np.diff(blocks["lanes_meta"][:P, 3]) >= 0).all() and (blocks["lanes_meta"][:P, 3] >= 0).all()
            dist = np.asarray([abs(lt) + max(lg - float(L["length"]), 0.0) + max(-lg, 0.0)
                               for L in lanes for lg, lt in [vh.lane_local(L, float(me["cx"]), float(me["cy"]))]], np.float32)
            order = np.lexsort((np.arange(len(lanes)), dist))[:P]
            assert np.array_equal(blocks["lanes_meta"][:P, 3], dist[order])
            assert blocks["lanes_meta"][:P, 2].tolist() == [float(int(lanes[i]["road"]) in road_ids) for i in order], (e, a)
            assert blocks["lanes_meta"][:P, 1].tolist() == [float(lanes[i]["length"]) for i in order]
            for p, i in enumerate(order):           # the polyline runs from the lane's start point to its end point
                for at, (px, py) in ((0, (lanes[i]["sx"], lanes[i]["sy"])), (-1, (lanes[i]["ex"], lanes[i]["ey"]))):
                    rx, ry = float(px) - float(me["cx"]), float(py) - float(me["cy"])
                    assert np.abs(blocks["lanes"][p, at] - [rx * c + ry * s, ry * c - rx * s]).max() < 1e-3, (e, a, p, at)
    return dict(clock=clock.copy(), near={k: v for k, v in now.items() if len(k) == 2},
                kinds={k[1:]: v for k, v in now.items() if len(k) == 3})


def _rollout(host, vo_cfg, steps, actions_of):
    import oracle_binding as ob
    orc = ob.OracleWorld(host)
    hv = vh.HostVectorObs(vo_cfg, host.E, host.A, host.cap)
    seen, prev = Seen(), None
    orc.reset()
    hv.run(orc.w, orc.s, orc.k)
    assert (hv.history()["cursor"][:, 1] == 1).all(), "a reset observation holds exactly one frame"
    for t in range(steps):
        orc.step(actions_of(t))
        hv.run(orc.w, orc.s, orc.k)
        prev = _check_invariants(host, orc.state, hv, hv.cfg, prev, seen)
    return seen


def test_invariants_single_agent_rollout():
    host = _pg_host(horizon=30, traffic_mode="respawn", agent_policy="EnvInputPolicy")
    seen = _rollout(host, dict(vh.SMALL, radius=20.0, route_spacing=8.0), 40, lambda t: scripted_actions(host.E, host.A, t))
    assert seen.enters >= 1 and seen.leaves >= 1, (seen.enters, seen.leaves)
    assert seen.onto_circle >= 1 and seen.resets >= 1, (seen.onto_circle, seen.resets)


def test_invariants_multi_agent_intersection_rollout():
    from metadrive_ped_amd.engine import HostScene
    from metadrive_ped_amd.envs import BatchedMultiAgentIntersectionEnv
    env = BatchedMultiAgentIntersectionEnv(dict(num_envs=1, horizon=30))
    host = HostScene(env.config)
    # env 0 of the scripted actions brakes: the one env here takes env 1's, which drive
    seen = _rollout(host, dict(vh.SMALL, radius=16.0, route_spacing=10.0), 40, lambda t: scripted_actions(2, host.A, t)[1:])
    assert seen.enters >= 1 and seen.leaves >= 1, (seen.enters, seen.leaves)
    assert seen.onto_circle >= 1 and seen.resets >= 1 and 0 < seen.invalid < seen.observers, vars(seen)


# -- 6. config and the env API without a device ----------------------------------------------------------------------------------------
def test_defaults_are_merged():
    assert make_config({})["vector_obs"] is None
    assert make_config(dict(vector_obs={}))["vector_obs"] == VECTOR_OBS_DEFAULT_CONFIG
    vo = make_config(dict(vector_obs=dict(num_agents=3, radius=25)))["vector_obs"]
    assert vo == dict(VECTOR_OBS_DEFAULT_CONFIG, num_agents=3, radius=25.0) and isinstance(vo["radius"], float)
    assert VECTOR_OBS_DEFAULT_CONFIG == dict(num_agents=8, history=5, radius=50.0, max_jump=8.0, route_points=16, route_spacing=4.0,
                                             num_lanes=8, lane_points=8)
    assert [vh.lib().hx_vo_limit(i) for i in range(5)] == [VECTOR_OBS_RANGES[k][1] for k in
                                                          ("num_agents", "history", "route_points", "num_lanes", "lane_points")]
    assert (abi.MD_VO_MAX_AGENTS, abi.MD_VO_MAX_HISTORY, abi.MD_VO_MAX_ROUTE_POINTS, abi.MD_VO_MAX_LANES, abi.MD_VO_MAX_LANE_POINTS) == \
        tuple(vh.lib().hx_vo_limit(i) for i in range(5))


@pytest.mark.parametrize("key,bad", [("num_agents", 0), ("num_agents", 17), ("history", 0), ("history", 9), ("route_points", -1),
                                     ("route_points", 33), ("num_lanes", -1), ("num_lanes", 17), ("lane_points", 1), ("lane_points", 17),
                                     ("num_agents", 2.0), ("history", True), ("radius", 0), ("radius", -1.0), ("max_jump", 0.0),
                                     ("route_spacing", 0), ("route_spacing", "4")])
def test_each_range_is_refused_with_the_key_s_name(key, bad):
    with pytest.raises(ValueError, match=r"vector_obs\['%s'\]" % key):
        make_config(dict(vector_obs={key: bad}))


def test_other_refusals():
    from metadrive_ped_amd.scenario import make_scenario_config
    with pytest.raises(ValueError, match="unknown key.*'pace'"):
        make_config(dict(vector_obs=dict(pace=1)))
    with pytest.raises(ValueError, match="vector_obs=True"):
        make_config(dict(vector_obs=True))
    with pytest.raises(NotImplementedError, match="vector_obs in BatchedScenarioEnv is not built"):
        make_scenario_config(dict(vector_obs={}))
    assert make_scenario_config({})["vector_obs"] is None


def test_every_other_family_and_mode_accepts_the_key():
    from metadrive_ped_amd import envs
    for cfg in (dict(traffic_mode="respawn"), dict(traffic_mode="hybrid"), dict(agent_policy="IDMPolicy"), dict(num_pedestrians=2),
                dict(walk_scenarios=True, num_scenarios=4), dict(random_traffic=True), dict(agent_policy="ExpertPolicy"),
                dict(agent_policy="LaneChangePolicy", discrete_action=True)):
        assert make_config(dict(cfg, vector_obs={}))["vector_obs"]["history"] == 5, cfg
    for name in ("BatchedMetaDriveEnv", "BatchedSafeMetaDriveEnv", "BatchedMultiAgentRoundaboutEnv", "BatchedMultiAgentIntersectionEnv",
                 "BatchedMultiAgentTollgateEnv", "BatchedMultiAgentBottleneckEnv", "BatchedMultiAgentParkingLotEnv",
                 "BatchedMultiAgentRacingEnv", "BatchedMultiAgentMetaDrive"):
        cls = getattr(envs, name, None)
        if cls is not None:
            assert cls(dict(num_envs=2, vector_obs=dict(history=2))).config["vector_obs"]["history"] == 2, name


def test_vector_obs_without_the_key_raises_and_the_spec_has_the_shapes():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv, BatchedMultiAgentRoundaboutEnv
    env = BatchedMetaDriveEnv(dict(num_envs=4))
    for fn in (env.vector_obs, env.vector_obs_spec):
        with pytest.raises(RuntimeError, match=r"config\['vector_obs'\] is None"):
            fn()
    env = BatchedMetaDriveEnv(dict(num_envs=4, vector_obs={}))
    f, b = np.float32, np.uint8
    assert env.vector_obs_spec() == dict(agents=((4, 8, 5, 4), f), agents_mask=((4, 8, 5), b), agents_meta=((4, 8, 4), f), ego=((4, 5, 4), f),
                                         ego_mask=((4, 5), b), route=((4, 16, 4), f), route_mask=((4, 16), b), lanes=((4, 8, 8, 2), f),
                                         lanes_meta=((4, 8, 4), f), lanes_mask=((4, 8), b))
    with pytest.raises(RuntimeError, match="call reset"):
        env.vector_obs()
    ma = BatchedMultiAgentRoundaboutEnv(dict(num_envs=2, num_agents=5, vector_obs=dict(vh.SMALL)))
    spec = ma.vector_obs_spec()
    assert spec["agents"] == ((2, 5, 3, 3, 4), f) and spec["lanes"] == ((2, 5, 3, 3, 2), f) and spec["route_mask"] == ((2, 5, 5), b)
    assert list(spec) == list(abi.VECTOR_OBS_OUTPUTS)


def test_the_engine_s_layout_is_one_row_per_env_with_aligned_blocks():
    outs, out_bytes, hist, hist_bytes = abi.vector_obs_blocks(dict(VECTOR_OBS_DEFAULT_CONFIG), 3, 24)
    assert out_bytes % 16 == 0 and hist_bytes % 16 == 0
    end = 0
    for table, total in ((outs, out_bytes), (hist, hist_bytes)):
        end = 0
        for name, (off, shape, dt) in table.items():
            assert off % 16 == 0 and off >= end, name
            end = off + int(np.prod(shape)) * dt.itemsize
        assert end <= total
    assert hist["ring_pose"][1] == (5, 24, 4) and hist["cursor"][1] == (4, )
