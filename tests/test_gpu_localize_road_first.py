"""The road-first localisation of the lean step kernel (csrc/parts/localize.inc, localize_road_first): a vehicle is first looked for on
the lanes of its route's current road, read straight from the lane table around its previous lane, and only then through the
grid.  Both ways must name the same lane, bit for bit with the oracle's scan over all lanes:
  (a) md_localize_road_first (the stand-alone localisation with the path on) against ref_localize on placed states,
  (b) md_step rollouts on maps too large to stage (the kernel that carries the path) against the oracle."""
import math

import numpy as np
import pytest

from helpers import assert_state_equal

pytestmark = pytest.mark.gpu

E = 8
SLOT = 0     # the agent's slot: the placed vehicle


def _engine_and_oracle(**kw):
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    import oracle_binding as ob
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    eng = BatchedEngine(make_config(dict(dict(num_envs=E, num_scenarios=E), **kw)))
    return eng, ob.OracleWorld(eng.host)


class Placed:
    """One placed state: pose, previous lane, the roads under the two route cursors (next < 0: the cursors coincide)"""
    def __init__(self, xy, heading, nav_lane, cur_road, next_road):
        self.xy, self.heading, self.nav_lane, self.cur_road, self.next_road = xy, heading, nav_lane, cur_road, next_road


def _on(mt, l, s, lat, nav_lane=None, cur_road=None, next_road=None, turn=0.0):
    lane = mt.lane_objs[l]
    road = int(mt.lanes["road"][l])
    if next_road is None:
        nxt = np.nonzero(mt.roads["start_node"] == mt.roads["end_node"][road])[0]
        next_road = int(nxt[0]) if len(nxt) else -1
    return Placed(lane.position(s, lat), lane.heading_theta_at(s) + turn, l if nav_lane is None else nav_lane,
                  road if cur_road is None else cur_road, next_road)


def _cases(mt, rng):
    """The placed states of one map, as (name, Placed)"""
    L, R = mt.lanes, mt.roads
    nl = len(L)
    out = []
    wide = [r for r in range(len(R)) if R["n_lanes"][r] >= 2]
    pick = lambda seq: int(seq[rng.randint(len(seq))])
    for _ in range(3):
        # the seam between two adjacent lanes of one road (distance ties), and the road's outer edges
        r = pick(wide)
        l = int(R["first_lane"][r]) + rng.randint(R["n_lanes"][r] - 1)
        w, ln = float(L["width"][l]), float(L["length"][l])
        s = rng.uniform(0.1, 0.9) * ln
        for lat in (0.5 * w, -0.5 * w, 0.0):
            out.append(("seam", _on(mt, l, s, lat)))
            out.append(("seam", _on(mt, l + 1, s, lat, nav_lane=l)))
        # the overlap of a road's last metres and the next road's first 5 m, seen from both roads' cursors
        nxt = [q for q in range(len(R)) if R["start_node"][q] == R["end_node"][r]]
        for q in nxt[:2]:
            lq = int(R["first_lane"][q]) + rng.randint(R["n_lanes"][q])
            for s_q in (-0.5, 0.0, 0.5, 2.0, 4.9, 5.1):
                out.append(("overlap", _on(mt, lq, s_q, 0.3, nav_lane=l, cur_road=r, next_road=q)))
            out.append(("overlap", _on(mt, l, ln - 0.5, 0.0, next_road=q)))
            out.append(("overlap", _on(mt, l, ln + 0.5, 0.0, next_road=q)))
        # heading reversed (the heading filter fails on the current road), and across the lane
        out.append(("reversed", _on(mt, l, s, 0.2, turn=math.pi)))
        out.append(("reversed", _on(mt, l, s, 0.2, turn=0.5 * math.pi)))
        # off every lane
        far = _on(mt, l, s, 0.0)
        far.xy = far.xy + np.array([3000.0, -2000.0])
        out.append(("off_lanes", far))
        out.append(("off_lanes", _on(mt, l, s, 60.0)))
        # the previous lane on a road other than road0; no previous lane
        other = pick([k for k in range(nl) if L["road"][k] != r])
        out.append(("other_road", _on(mt, l, s, 0.4, nav_lane=other)))
        out.append(("no_lane", _on(mt, l, s, 0.4, nav_lane=-1)))
    # a circular lane inside the chord region that its neighbour's hull also covers
    circ = [k for k in range(nl) if L["type"][k] == 1 and L["n_in_road"][k] >= 2]
    for _ in range(4 if circ else 0):
        l = pick(circ)
        w, ln = float(L["width"][l]), float(L["length"][l])
        for frac in (0.1, 0.5, 0.9):
            for lat in (-1.4 * w, -0.9 * w, -0.5 * w, 0.0, 0.5 * w, 0.9 * w, 1.4 * w):
                out.append(("chord", _on(mt, l, frac * ln, lat)))
    # the previous lane at the first and at the last lane id of the map: the window is clamped to the map's lanes
    for l in (0, nl - 1):
        for lat in (0.0, 0.5 * float(L["width"][l])):
            out.append(("map_edge", _on(mt, l, 0.5 * float(L["length"][l]), lat)))
    return out


def _place(state, base, cap, placed):
    """Write one Placed per env into the state arrays (restored from `base` first)"""
    for k in ("shape", "nav", "flags", "route_roads"):
        state[k][...] = base[k]
    rr = state["route_roads"].reshape(E * cap, -1)
    for e, p in enumerate(placed):
        n = e * cap + SLOT
        sh, nav = state["shape"], state["nav"]
        sh["cx"][n], sh["cy"][n] = np.float32(p.xy[0]), np.float32(p.xy[1])
        sh["c"][n], sh["s"][n] = np.float32(math.cos(p.heading)), np.float32(math.sin(p.heading))
        has_next = p.next_road >= 0
        nav["lane"][n], nav["ck0"][n], nav["ck1"][n] = p.nav_lane, 0, 1 if has_next else 0
        rr[n, 0] = p.cur_road
        if has_next:
            rr[n, 1] = p.next_road
        nav["road0"][n], nav["road1"][n] = rr[n, 0], rr[n, nav["ck1"][n]]


@pytest.mark.parametrize("name,seq", [("intersection", "X"), ("roundabout", "O"), ("curve", "C"), ("t_intersection_ramp", "TR")])
def test_localize_road_first_matches_oracle_on_placed_states(name, seq):
    from metadrive_ped_amd import abi
    eng, orc = _engine_and_oracle(map=seq, traffic_density=0.0, mover_capacity=8, auto_reset=False)
    assert hasattr(eng.lib, "md_localize_road_first")
    eng.reset()
    orc.reset()
    cap = eng.cap
    base = {k: v.copy() for k, v in orc.state.items()}
    assert_state_equal(eng.download_state(), base, where=name + " reset")
    drives = base["shape"]["flags"].reshape(E, cap)[:, SLOT]
    assert ((drives & abi.KIND_MASK) == abi.KIND_VEHICLE).all() and not (drives & (abi.F_STATIC | abi.F_PENDING)).any()
    env_map = eng.host.world.arrays["env_map"]
    rng = np.random.RandomState(5)
    per_env = [_cases(eng.host.map_tables[int(env_map[e])], rng) for e in range(E)]
    kinds = set(k for c in per_env for k, _ in c)
    want = {"seam", "overlap", "reversed", "off_lanes", "other_road", "no_lane", "map_edge"} | ({"chord"} if seq in "OCX" else set())
    assert want <= kinds, (name, kinds)
    rounds = max(len(c) for c in per_env)
    on_lane = changed = advanced = 0
    for r in range(rounds):
        placed = [c[r % len(c)] for c in per_env]
        _place(orc.state, base, cap, [p for _, p in placed])
        eng.upload_state({k: orc.state[k] for k in ("shape", "nav", "flags", "route_roads")})
        before = orc.state["nav"].copy()
        eng.call("md_localize_road_first")
        orc.call("ref_localize")
        got = eng.download_state()
        where = "%s round %d (%s)" % (name, r, ",".join(k for k, _ in placed))
        assert_state_equal(got, orc.state, keys=["nav", "flags", "shape"], where=where)
        rows = np.arange(E) * cap + SLOT
        on_lane += int(((orc.state["flags"][rows] & abi.FL_ON_LANE) != 0).sum())
        changed += int((orc.state["nav"]["lane"][rows] != before["lane"][rows]).sum())
        advanced += int((orc.state["nav"]["ck0"][rows] != before["ck0"][rows]).sum())
    # the placed states must have reached every outcome: on and off the lanes, lane changes, cursor advances
    assert on_lane > rounds and on_lane < rounds * E and changed > 0 and advanced > 0, (on_lane, changed, advanced)


def _lane_follow_actions(orc, eng, t, random_envs):
    """Steer the agents along their current lane (they cross road boundaries); `random_envs` act at random and leave the road"""
    cap = eng.cap
    a = np.zeros((E, 1, 2), np.float32)
    env_map = eng.host.world.arrays["env_map"]
    rng = np.random.RandomState(977 + t)
    for e in range(E):
        n = e * cap + SLOT
        if e in random_envs:
            a[e, 0] = rng.uniform(-1, 1, 2)
            a[e, 0, 1] = abs(a[e, 0, 1])
            continue
        sh, l = orc.state["shape"][n], int(orc.state["nav"]["lane"][n])
        steer = 0.0
        if l >= 0:
            lane = eng.host.map_tables[int(env_map[e])].lane_objs[l]
            s, lat = lane.local_coordinates((float(sh["cx"]), float(sh["cy"])))
            err = math.atan2(float(sh["s"]), float(sh["c"])) - lane.heading_theta_at(min(max(s, 0.0), lane.length))
            err = (err + math.pi) % (2 * math.pi) - math.pi
            # lat > 0: right of the centre line, so steer left (positive); heading error the same way
            steer = max(-1.0, min(1.0, 0.3 * lat + 1.5 * err))
        a[e, 0] = (steer, 0.6 if float(orc.state["dyn"]["speed"][n]) < 12.0 else 0.0)
    return a


@pytest.mark.parametrize("auto_reset", [False, True])
def test_step_rollout_road_first_parity(auto_reset):
    """300 md_step steps of the lean kernel on the default block distribution (intersections, roundabouts, curves, ramps: lane
    tables too large to stage), lane-following and random agents, traffic on"""
    import torch
    from metadrive_ped_amd import abi
    eng, orc = _engine_and_oracle(start_seed=100, traffic_density=0.3, auto_reset=auto_reset, horizon=220)
    assert eng.w.max_lanes > 64 and eng.host.step_kernel == "wg", "the batch must take the non-staged workgroup kernel"
    blocks = set(b.ID for mt in eng.host.map_tables for b in mt.pg_map.blocks)
    assert {"X", "O", "C"} <= blocks or {"T", "O", "C"} <= blocks, blocks
    eng.reset()
    orc.reset()
    assert_state_equal(eng.download_state(), orc.state, where="reset")
    random_envs = (2, 5)
    roads_seen = [set() for _ in range(E)]
    off = left = paired = 0
    for t in range(300):
        a = _lane_follow_actions(orc, eng, t, random_envs)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        if t % 10 == 0:
            assert_state_equal(eng.download_state(), orc.state, where="step %d" % t)
        rows = np.arange(E) * eng.cap + SLOT
        for e in range(E):
            roads_seen[e].add(int(orc.state["nav"]["road0"][rows[e]]))
        off += int(((orc.state["flags"][rows] & abi.FL_ON_LANE) == 0).sum())
        left += int(((orc.state["flags"][rows] & abi.FL_OUT_OF_ROAD) != 0).sum())
        fl = orc.state["shape"]["flags"].reshape(E, -1)
        drives = ((fl & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((fl & abi.F_ALIVE) != 0) & ((fl & (abi.F_STATIC | abi.F_PENDING)) == 0)
        paired += int((drives.sum(1) >= 4).sum())
    assert_state_equal(eng.download_state(), orc.state, where="final")
    followers = [e for e in range(E) if e not in random_envs]
    assert sum(len(roads_seen[e]) >= 3 for e in followers) >= len(followers) // 2, roads_seen   # they crossed road boundaries
    assert left > 0, "no agent ever left the road"
    assert paired > 100, "too few env-steps with four or more driving vehicles: the two-per-wave form was hardly reached"
    if not auto_reset:     # (an auto-reset env starts over before its vehicle is off every lane)
        assert off > 0, "no agent was ever off every lane"
