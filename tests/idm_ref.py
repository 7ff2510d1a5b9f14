"""Float64 reference of one vehicle's IDM step (md_idm_vehicle of include/md_entity.h: stage A md_idm_plan, stage B
md_find_front_back with md_idm_is_candidate / md_idm_sees_participant / md_fb_same_lane_gap / md_fb_neighbour, stage C
md_idm_policy and md_idm_act) on a downloaded state, and the placed cases its tests share.  TEST INFRASTRUCTURE, numpy only:
it calls none of the C code.

What is restated.  The documented semantics of the three stages, in float64, on the float32 records the kernel reads (shape,
dyn, nav, pid, aux, idm_rand).  Every projection goes through the Python lane objects of mapgen/lanes.py
(`local_coordinates`, `heading_theta_at`, float64), never through md_lane_local; lane lengths and the lane graph
(is_previous_lane_of) come from the same objects.  A body is a candidate when it is present, is not the vehicle itself and
touches the 50 m circle (an OBB, or for the circle kinds a radius of hl); a pedestrian or cyclist among the candidates gives the
fallback (no front object, distance 5, steering on the target lane).  Front / back per scanned lane in the canonical form:
same-lane objects first (front in (0, 30), back |gap| < 30), connected-lane objects only for the buckets the same lane left
empty (front in (0, 30), back < 30 with negative gaps allowed; the front is chosen before the back), ties to the lowest slot.

Decidedness.  Every comparison that branches records its margin: a gap against 0 and 30, the best against the runner-up of a
bucket, the 50 m ring, 15 m and 5 m in the lane-change tests, the +-3 km/h and +10 km/h speed tests, the d_start > d_end branch
of a circular lane's projection (as an arc length) and wrap_to_pi near +-pi (projections: as an arc length; the heading error:
in radians).  A vehicle is decided when every margin it passed exceeds MARGIN.  Two gaps of one bucket that agree to TIE_EPS in
float64 are a tie and go to the lowest slot (the `tie` family asserts that the float32 gaps are bit-equal there).

Sensitivity.  For every bucket the action is evaluated again with the bucket's runner-up in the winner's place and with the
bucket empty; `Result.sens[(lane index, "front" | "back", "runner" | "none")]` = (|d steering|, |d acceleration|, discrete
fields changed).  A named case names the bucket it is about and the word that carries it, and must show at least
SENS_FACTOR x the tolerance there.  Only what the policy reads can show: the own lane's back bucket is never read, and a side
lane's back gap only against 15 m -- the back families therefore run on a side lane in the overtake situation, and a back
runner-up on the same side of 15 m as the winner cannot show (such cases assert the "none" variant only).

Constants, MEASURED on the CPU (tests/test_idm_ref.py::test_constants_are_the_measured_ones prints the numbers and asserts
them), never from the device:
    MARGIN     4 x the largest |ref_lane_local - float64 projection| over every projection the cases need (every body and ego
               on every lane it is projected on, all launch sets of the device test): longitudinal 2.46e-5 m (a circular lane of
               the roundabout; straight lanes 8e-6 m), lateral 6.1e-6 m -> 4 x = 9.8e-5 m -> MARGIN = 1e-4 m (rounded up to one
               digit of 1, 2, 5).  A gap is the difference of two projections, doubled again for headroom.  Sanity cap 1 cm.
    TOL_STEER  4 x the largest |oracle - float64| of the steering word over all decided vehicles of all cases (1130): 3.8e-6
               (a curve family of the roundabout) -> 1.5e-5 -> 2e-5
    TOL_ACC    the same for the acceleration word, RELATIVE to max(1, |acc|): 3.5e-6 -> 1.4e-5 -> 2e-5.  Relative, because the
               word is (desired gap / front distance)^2: a cone half a metre ahead (the window family) gives -6000, where one
               float32 ulp is 5e-4.  For the same reason the random fill keeps its bodies 6 m apart: at a front distance of
               0.76 m the 2e-5 m of a projection alone are 5e-5 of the word.
    Undecided  at most UNDECIDED_CAP = 5 % of the driving vehicles of any one test, none among the named cases: placements keep
               0.3 m from every threshold.  Measured on the reference alone: 0 % in every launch set.
"""
import math

import numpy as np

import contact_ref as cr
from metadrive_ped_amd import abi

MARGIN = 1.0e-4
MARGIN_CAP = 1.0e-2
TOL_STEER = 2.0e-5
TOL_ACC = 2.0e-5
SENS_FACTOR = 100.0
UNDECIDED_CAP = 0.05
TIE_EPS = 1.0e-9
RING = 50.0
MAX_LONG, SAFE_CHANGE, LANE_CHANGE_FREQ, SPEED_INC = 30.0, 15.0, 50, 10.0
NORMAL_SPEED, CREEP_SPEED, MAX_SPEED = 30.0, 5.0, 100.0
ALIVE, STATIC = abi.F_ALIVE, abi.F_STATIC
PARTICIPANTS = (abi.KIND_PEDESTRIAN, abi.KIND_CYCLIST)
# kind -> (hl, hw, shape flags)
BODIES = {"vehicle": (2.2, 0.9, abi.KIND_VEHICLE | ALIVE | STATIC),
          "cone": (0.2, 0.2, abi.KIND_CONE | ALIVE | STATIC),
          "warning": (0.25, 0.25, abi.KIND_WARNING | ALIVE | STATIC),
          "barrier": (0.15, 1.0, abi.KIND_BARRIER | ALIVE | STATIC),
          "pedestrian": (0.35, 0.35, abi.KIND_PEDESTRIAN | ALIVE),
          "cyclist": (0.875, 0.2, abi.KIND_CYCLIST | ALIVE)}
MOVING = abi.KIND_VEHICLE | ALIVE
DISCRETE = ("target_lane", "timer", "rand_cursor", "target_speed")


def _f(v):
    return float(v)


def wrap_to_pi(x):
    a = x % (2.0 * math.pi)
    return a - 2.0 * math.pi if a > math.pi else a


def _seam(x):
    """how far x lies from the +-pi seam of wrap_to_pi"""
    return abs(abs(wrap_to_pi(x)) - math.pi)


def present(flags):
    return bool(int(flags) & ALIVE) and (int(flags) & abi.KIND_MASK) != abi.KIND_NONE


def kind_of(flags):
    return int(flags) & abi.KIND_MASK


def drives(flags):
    f = int(flags)
    return present(f) and kind_of(f) == abi.KIND_VEHICLE and not f & (STATIC | abi.F_PENDING)


class MapRef:
    """One map's lane objects and graph, float64"""
    def __init__(self, mt, enable_lane_change=1):
        self.mt = mt
        self.objs = mt.lane_objs
        self.n = len(self.objs)
        self.road_of = [int(r) for r in mt.lanes["road"]]
        self.idx_of = [int(r) for r in mt.lanes["idx"]]
        self.roads = mt.roads
        self.enable_lane_change = int(enable_lane_change)
        self.log = None      # a list: every projection asked for is appended, (lane, x, y, longitudinal, lateral)
        ends = np.asarray([l.end for l in self.objs], np.float64)
        starts = np.asarray([l.start for l in self.objs], np.float64)
        d = np.sqrt(((ends[:, None] - starts[None]) ** 2).sum(-1))      # d[a, b]: end of a to start of b
        self.prev = d < 0.1                                             # prev[a, b]: a is a previous lane of b
        self.graph_margin = float(np.abs(d - 0.1).min())
        self.succ = [[int(b) for b in np.nonzero(self.prev[a])[0]] for a in range(self.n)]
        self.pred = [[int(a) for a in np.nonzero(self.prev[:, b])[0]] for b in range(self.n)]

    def road_connects(self, a, b):
        off, adj = self.mt.node_adj_off, self.mt.node_adj
        return any(int(adj[k][0]) == b for k in range(int(off[a]), int(off[a + 1])))

    def project(self, l, x, y, margins=None):
        """(longitudinal, lateral) of the lane object; a circular lane adds the margins of its branches, as arc lengths"""
        L = self.objs[l]
        s, lat = L.local_coordinates((x, y))
        if self.log is not None:
            self.log.append((l, x, y, float(s), float(lat)))
        if margins is not None and L.kind == 1:
            ph = math.atan2(y - L.center[1], x - L.center[0])
            d_start, d_end = abs(wrap_to_pi(ph - L.start_phase)), abs(wrap_to_pi(ph - L.end_phase))
            margins.append(("arc_branch", abs(d_start - d_end) * L.radius))
            ref = L.end_phase if d_start > d_end else L.start_phase
            margins.append(("arc_seam", _seam(ph - ref) * L.radius))      # (|wrap| of d_start / d_end is continuous across its seam)
        return float(s), float(lat)

    def neighbours(self, l):
        """(left, right) lane ids on l's road, -1: none"""
        r = self.roads[self.road_of[l]]
        i = self.idx_of[l]
        return (l - 1 if i > 0 else -1), (l + 1 if i + 1 < int(r["n_lanes"]) else -1)


class Result:
    pass


def ring_distance(o, px, py):
    """the body's distance to the 50 m circle around (px, py): <= 0 touches"""
    dx, dy = px - _f(o["cx"]), py - _f(o["cy"])
    if kind_of(o["flags"]) in cr.CIRCLE_KINDS:
        return math.hypot(dx, dy) - (RING + _f(o["hl"]))
    c, s = _f(o["c"]), _f(o["s"])
    lx = max(abs(dx * c + dy * s) - _f(o["hl"]), 0.0)
    ly = max(abs(dy * c - dx * s) - _f(o["hw"]), 0.0)
    return math.hypot(lx, ly) - RING


def obj_lane(env, j):
    f = int(env["shape"]["flags"][j])
    if kind_of(f) == abi.KIND_VEHICLE and not f & STATIC:
        return int(env["nav"]["lane"][j])
    return int(env["shape"]["aux"][j])


def _pick(entries, margins):
    """entries [(gap, slot)] -> the winner (smallest gap, ties to the lowest slot), the runner-up"""
    if not entries:
        return None, None
    g0 = min(g for g, _ in entries)
    tied = sorted(j for g, j in entries if g - g0 <= TIE_EPS)
    rest = sorted((g, j) for g, j in entries if g - g0 > TIE_EPS)
    if rest:
        margins.append(("runner_up", rest[0][0] - g0))
    best = (g0, tied[0])
    runner = (g0, tied[1]) if len(tied) > 1 else (rest[0] if rest else None)
    return best, runner


def plan(mr, env, slot, idm_rand):
    """stage A -> dict(target_lane, timer, rand_cursor, success, fail, use_ref, ids)"""
    nav = env["nav"][slot]
    lane, road0, target, timer, cursor = (int(nav[k]) for k in ("lane", "road0", "target_lane", "timer", "rand_cursor"))
    cur = mr.roads[road0]
    in_cur = lane >= 0 and mr.road_of[lane] == road0
    if target < 0:
        target, success = lane, in_cur
    elif mr.road_of[target] != road0:
        success = False
        t_end = int(mr.roads[mr.road_of[target]]["end_node"])
        for k in range(int(cur["n_lanes"])):
            l = int(cur["first_lane"]) + k
            if mr.prev[target, l] or mr.road_connects(t_end, int(cur["end_node"])):
                target, success = l, True
                break
    elif in_cur and target != lane:
        target = lane
        timer = int(idm_rand[cursor % abi.MD_IDM_RAND])
        cursor += 1
        success = True
    else:
        success = True
    fail = target < 0
    use_ref = bool(success) and bool(mr.enable_lane_change)
    ids = [-1, target, -1]
    if not fail and use_ref:
        i = mr.idx_of[target]
        if i > 0:
            ids[0] = int(cur["first_lane"]) + i - 1
        if i + 1 < int(cur["n_lanes"]):
            ids[2] = int(cur["first_lane"]) + i + 1
    return dict(target_lane=target, timer=timer, rand_cursor=cursor, success=bool(success), fail=fail, use_ref=use_ref, ids=ids)


def candidates(env, slot, margins):
    """-> (slots that touch the ring, a participant among them)"""
    sh = env["shape"]
    px, py = _f(sh["cx"][slot]), _f(sh["cy"][slot])
    out, participant = [], False
    for j in range(len(sh)):
        if j == slot or not present(sh["flags"][j]):
            continue
        d = ring_distance(sh[j], px, py)
        margins.append(("ring", abs(d)))
        if d <= 0.0:
            out.append(j)
            participant |= kind_of(sh["flags"][j]) in PARTICIPANTS
    return out, participant


def front_back(mr, env, slot, ids, cand, margins):
    """stage B -> {(i, "front" | "back"): (best, runner)}, best / runner = (gap, slot) or None; exist[3]"""
    sh = env["shape"]
    px, py = _f(sh["cx"][slot]), _f(sh["cy"][slot])
    out = {}
    for i in range(3):
        out[(i, "front")] = out[(i, "back")] = (None, None)
        l = ids[i]
        if l < 0:
            continue
        cur_long = mr.project(l, px, py, margins)[0]
        left_long = mr.objs[l].length - cur_long
        fronts, backs = [], []
        for j in cand:
            if obj_lane(env, j) != l:
                continue
            lg = mr.project(l, _f(sh["cx"][j]), _f(sh["cy"][j]), margins)[0] - cur_long
            margins += [("gap_0", abs(lg)), ("gap_30", abs(abs(lg) - MAX_LONG))]
            if 0.0 < lg < MAX_LONG:
                fronts.append((lg, j))
            if lg < 0.0 and -lg < MAX_LONG:
                backs.append((-lg, j))
        need_front, need_back = not fronts, not backs
        if need_front or need_back:
            for j in cand:
                ol = obj_lane(env, j)
                if ol < 0 or ol == l:
                    continue
                if need_front and mr.prev[l, ol]:
                    lg = mr.project(ol, _f(sh["cx"][j]), _f(sh["cy"][j]), margins)[0] + left_long
                    margins += [("gap_0", abs(lg)), ("gap_30", abs(lg - MAX_LONG))]
                    if 0.0 < lg < MAX_LONG:
                        fronts.append((lg, j))
                elif need_back and mr.prev[ol, l]:
                    lg = mr.objs[ol].length - mr.project(ol, _f(sh["cx"][j]), _f(sh["cy"][j]), margins)[0] + cur_long
                    margins.append(("gap_30", abs(lg - MAX_LONG)))
                    if lg < MAX_LONG:
                        backs.append((lg, j))
        out[(i, "front")] = _pick(fronts, margins)
        out[(i, "back")] = _pick(backs, margins)
    return out


def _fb_of(buckets, ids, fail):
    """the FrontBack record stage C reads"""
    fb = dict(front=[-1] * 3, back=[-1] * 3, front_d=[MAX_LONG] * 3, back_d=[MAX_LONG] * 3, exist=[l >= 0 and not fail for l in ids])
    for (i, side), best in buckets.items():
        if best is not None:
            fb[side][i], fb[side + "_d"][i] = best[1], best[0]
    return fb


def policy(mr, env, slot, pl, fb, margins):
    """stage C, first half -> dict(timer, target_speed, steer_lane, front_obj, front_dist)"""
    nav, dyn = env["nav"][slot], env["dyn"]
    cur = mr.roads[int(nav["road0"])]
    has_next = int(nav["ck1"]) != int(nav["ck0"])
    nxt = mr.roads[int(nav["road1"])] if has_next else None
    speed_kmh = abs(_f(dyn["speed"][slot])) * 3.6
    target, timer = pl["target_lane"], pl["timer"]
    target_speed = _f(env["pid"]["target_speed"][slot])
    kmh = lambda j: abs(_f(dyn["speed"][j])) * 3.6
    front_obj, front_dist, steer, fail = -1, 5.0, target, pl["fail"]

    def blocked(i):
        margins.extend([("safe_15", abs(fb["back_d"][i] - SAFE_CHANGE)), ("front_5", abs(fb["front_d"][i] - 5.0))])
        return fb["back_d"][i] < SAFE_CHANGE or fb["front_d"][i] < 5.0

    def free(i):
        if not fb["exist"][i]:
            return False
        margins.extend([("safe_15", abs(fb["front_d"][i] - SAFE_CHANGE)), ("safe_15", abs(fb["back_d"][i] - SAFE_CHANGE))])
        return fb["front_d"][i] > SAFE_CHANGE and fb["back_d"][i] > SAFE_CHANGE

    if not fail:
        if pl["use_ref"]:
            ncur = int(cur["n_lanes"])
            lo, hi = 0, ncur - 1
            diff = ncur - int(nxt["n_lanes"]) if has_next else 0
            tidx = mr.idx_of[target]
            first = int(cur["first_lane"])
            decided = False
            if diff > 0:
                if mr.prev[first, int(nxt["first_lane"])]:
                    lo, hi = 0, int(nxt["n_lanes"]) - 1
                else:
                    lo, hi = diff, ncur - 1
                if tidx < lo or tidx > hi:
                    i, to = (0, tidx - 1) if tidx > hi else (2, tidx + 1)
                    if not fb["exist"][i]:
                        fail = True
                    elif blocked(i):
                        target_speed = CREEP_SPEED
                        front_obj, front_dist, steer = fb["front"][1], fb["front_d"][1], target
                    else:
                        target_speed = NORMAL_SPEED
                        front_obj, front_dist, steer = fb["front"][i], fb["front_d"][i], first + to
                    decided = True
            if not decided and not fail:
                overtake = False
                margins.append(("speed_3", abs(abs(speed_kmh - NORMAL_SPEED) - 3.0)))
                if abs(speed_kmh - NORMAL_SPEED) > 3.0 and fb["front"][1] >= 0:
                    margins.append(("speed_3", abs(abs(kmh(fb["front"][1]) - NORMAL_SPEED) - 3.0)))
                    overtake = abs(kmh(fb["front"][1]) - NORMAL_SPEED) > 3.0 and timer > LANE_CHANGE_FREQ
                if overtake:
                    front_sp = kmh(fb["front"][1])
                    right_sp = kmh(fb["front"][2]) if fb["front"][2] >= 0 else (MAX_SPEED if free(2) else -1.0)
                    left_sp = kmh(fb["front"][0]) if fb["front"][0] >= 0 else (MAX_SPEED if free(0) else -1.0)
                    for i, sp, ex in ((0, left_sp, tidx - 1), (2, right_sp, tidx + 1)):
                        if decided or sp < 0.0:
                            continue
                        margins.append(("speed_10", abs(sp - front_sp - SPEED_INC)))
                        if sp - front_sp > SPEED_INC and lo <= ex <= hi:
                            front_obj, front_dist, steer = fb["front"][i], fb["front_d"][i], first + ex
                            decided = True
                if not decided:
                    target_speed = NORMAL_SPEED
                    timer += 1
                    front_obj, front_dist, steer = fb["front"][1], fb["front_d"][1], target
        else:
            front_obj, front_dist, steer = fb["front"][1], fb["front_d"][1], target
    if fail:
        front_obj, front_dist, steer = -1, 5.0, target
    return dict(timer=timer, target_speed=target_speed, steer_lane=steer, front_obj=front_obj, front_dist=front_dist)


def _not_zero(x, eps):
    return x if abs(x) > eps else (eps if x > 0.0 else -eps)


def act(mr, env, slot, po, margins):
    """stage C, second half -> (steering, acceleration)"""
    if po["steer_lane"] < 0:
        return 0.0, 0.0
    sh, dyn, pid = env["shape"], env["dyn"], env["pid"][slot]
    px, py = _f(sh["cx"][slot]), _f(sh["cy"][slot])
    tl_s, tl_lat = mr.project(po["steer_lane"], px, py, margins)
    diff = mr.objs[po["steer_lane"]].heading_theta_at(tl_s + 1.0) - _f(dyn["heading"][slot])
    margins.append(("heading_seam", _seam(diff)))

    def pid_term(p, i, kp, ki, kd, err):
        return -kp * err - ki * (_f(pid[i]) + err) - kd * (err - _f(pid[p]))
    steering = pid_term("hp", "hi", 1.7, 0.01, 3.5, -wrap_to_pi(diff)) + pid_term("lp", "li", 0.3, 0.002, 0.05, -tl_lat)
    speed = _f(dyn["speed"][slot])
    speed_kmh = abs(speed) * 3.6
    c, s = _f(sh["c"][slot]), _f(sh["s"][slot])
    acc = 1.0 - (max(speed_kmh, 0.0) / _not_zero(po["target_speed"], 0.0)) ** 10
    j = po["front_obj"]
    if j >= 0:
        fv = _f(dyn["speed"][j]) if kind_of(sh["flags"][j]) == abi.KIND_VEHICLE else 0.0
        dv = (speed * c - fv * _f(sh["c"][j])) * 3.6 * c + (speed * s - fv * _f(sh["s"][j])) * 3.6 * s
        gap = 10.0 + speed_kmh * 1.5 + speed_kmh * dv / (2.0 * math.sqrt(5.0))
        acc -= (gap / _not_zero(po["front_dist"], 1.0e-2)) ** 2
    return steering, acc


def evaluate(mr, env, slot, idm_rand, sensitivity=True):
    """One vehicle's IDM step on env = {shape, dyn, nav, pid} rows of ONE env, idm_rand: the slot's row -> Result"""
    r = Result()
    margins = r.margins = []
    pl = r.plan = plan(mr, env, slot, idm_rand)
    cand, participant = candidates(env, slot, margins)
    r.cand, r.participant = cand, participant
    fail = pl["fail"] or participant
    pl = dict(pl, fail=fail)
    buckets = front_back(mr, env, slot, pl["ids"], cand, margins) if not fail else {}
    r.buckets = buckets
    r.fb = _fb_of({k: v[0] for k, v in buckets.items()}, pl["ids"], fail)
    po = r.policy = policy(mr, env, slot, pl, r.fb, margins)
    r.steering, r.acc = act(mr, env, slot, po, margins)
    r.target_lane, r.rand_cursor, r.timer, r.target_speed = pl["target_lane"], pl["rand_cursor"], po["timer"], po["target_speed"]
    r.margin = min([m for _, m in margins] + [math.inf])
    r.decided = r.margin > MARGIN
    r.sens = {}
    if sensitivity:
        for (i, side), (best, runner) in buckets.items():
            if best is None:
                continue
            for tag, other in (("runner", runner), ("none", None)):
                if tag == "runner" and runner is None:
                    continue
                alt = {k: v[0] for k, v in buckets.items()}
                alt[(i, side)] = other
                scratch = []
                po2 = policy(mr, env, slot, pl, _fb_of(alt, pl["ids"], fail), scratch)
                st2, acc2 = act(mr, env, slot, po2, scratch)
                r.sens[(i, side, tag)] = (abs(st2 - r.steering), abs(acc2 - r.acc),
                                          (po2["timer"], po2["target_speed"]) != (po["timer"], po["target_speed"]))
    return r


def acc_tol(acc):
    return TOL_ACC * max(1.0, abs(acc))


def env_rows(state, e, cap):
    return {k: state[k][e * cap:(e + 1) * cap] for k in ("shape", "dyn", "nav", "pid")}


def driving_slots(env, A=1):
    """the slots ref_idm runs: the driving vehicles that are no agents"""
    fl = env["shape"]["flags"]
    return [j for j in range(A, len(fl)) if drives(fl[j]) and not int(fl[j]) & abi.F_AGENT]


# --------------------------------------------------------------------------------------------------
# nav templates: one record per lane, as the engine produced it
# --------------------------------------------------------------------------------------------------
class Template:
    """what the engine held for one driving vehicle: its nav record with the route the cursors of that record walk"""
    def __init__(self, nav, route_roads, route_nodes, final_lane):
        self.nav, self.route_roads, self.route_nodes, self.final_lane = nav, route_roads, route_nodes, final_lane
        assert int(nav["road0"]) == int(route_roads[int(nav["ck0"])]) and int(nav["road1"]) == int(route_roads[int(nav["ck1"])])


def harvest_templates(seq, steps=150, envs=4):
    """{lane id: Template} from a short oracle-only rollout with respawning traffic on the map of block sequence `seq`: the
    records of driving traffic whose target lane is the lane it stands on, on its current road"""
    import oracle_binding as ob
    from helpers import scripted_actions
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(make_config(dict(num_envs=envs, num_scenarios=1, traffic_density=0.3, traffic_mode="respawn", mover_capacity=128,
                                      auto_reset=False, map=seq)))
    o = ob.OracleWorld(host)
    o.reset()
    lanes = host.map_tables[0].lanes
    seen = {}
    for t in range(steps):
        o.step(scripted_actions(envs, 1, t))
        sh, nav = o.state["shape"], o.state["nav"]
        f = sh["flags"]
        ok = ((f & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((f & ALIVE) != 0) & ((f & (STATIC | abi.F_PENDING | abi.F_AGENT)) == 0)
        ok &= (nav["lane"] >= 0) & (nav["lane"] == nav["target_lane"])
        for n in np.nonzero(ok)[0]:
            l = int(nav["lane"][n])
            if l not in seen and int(lanes["road"][l]) == int(nav["road0"][n]):
                seen[l] = Template(nav[n].copy(), o.state["route_roads"][n].copy(), o.state["route_nodes"][n].copy(), int(o.state["final_lane"][n]))
    return host.map_tables[0], seen


_TEMPLATES = {}


def templates(seq):
    if seq not in _TEMPLATES:
        _TEMPLATES[seq] = harvest_templates(seq)
    return _TEMPLATES[seq]


# --------------------------------------------------------------------------------------------------
# placed cases
# --------------------------------------------------------------------------------------------------
class Case:
    """One placed env: the agent's record (slot 0, moved out of everybody's ring), bodies [(slot, shape record)], rows {state key:
    [(slot, record)]} written after the shapes, and for a named case `about`: [dict(ego, bucket, winner, word, variants)] -- what
    the float64 reference must say before any launch"""
    def __init__(self, name, agent, bodies, rows, about=()):
        self.name, self.agent, self.bodies, self.rows, self.about = name, agent, list(bodies), rows, list(about)

    @property
    def family(self):
        return self.name.split(":")[0]


class Builder:
    """Places vehicles and bodies on the lanes of one map.  me0: the agent's record after the reset; rest: every speed 0 (the
    md_step runs: nothing may move before the planned-ahead IDM reads the state)"""
    def __init__(self, mr, tmpl, me0, cap=128, rest=False, seed=5, base_env=None):
        self.mr, self.tmpl, self.cap, self.rest = mr, tmpl, cap, rest
        self.base_env = base_env      # {shape, dyn, nav, pid} rows of one env of the base state: what a map puts there (toll booths) counts
        self.rng = np.random.RandomState(seed)
        g = mr.mt.grid[0]
        self.agent = me0.copy()
        self.agent["cx"], self.agent["cy"] = float(g["x0"]) - 60.0, float(g["y0"]) - 60.0      # beyond everybody's ring
        self.idm_rand = idm_rand_table(cap)

    # -- records --
    def pose(self, l, s, lat=0.0):
        L = self.mr.objs[l]
        p = L.position(s, lat)
        return float(p[0]), float(p[1]), float(L.heading_theta_at(s))

    def body(self, kind, l, s, lat=0.0, aux=None, flags=None, speed=0.0, turn=0.0):
        """a body of `kind` at (s, lat) of lane l, carrying the lane in aux -> (shape record, rows)"""
        hl, hw, fl = BODIES[kind]
        x, y, th = self.pose(l, s, lat)
        rec = cr.make_shapes([x], [y], np.asarray([th + turn]), hl, hw, fl if flags is None else flags)[0]
        rec["aux"] = l if aux is None else aux
        dyn = np.zeros(1, abi.DYN_DT)[0]
        dyn["heading"], dyn["speed"] = th + turn, 0.0 if self.rest else speed
        dyn["last_x"], dyn["last_y"], dyn["last_c"], dyn["last_s"] = rec["cx"], rec["cy"], rec["c"], rec["s"]
        return rec, {"dyn": dyn}

    def mover(self, l, s, lat=0.0, speed=5.0, timer=0, nav_lane=None, aux=-1, target=None):
        """a driving vehicle on template lane l -> (shape record, rows)"""
        rec, rows = self.body("vehicle", l, s, lat, aux=aux, flags=MOVING, speed=speed)
        t = self.tmpl[l]
        nav = t.nav.copy()
        nav["timer"], nav["rand_cursor"], nav["steps"], nav["done"] = timer, 0, 0, 0
        if nav_lane is not None:
            nav["lane"] = nav_lane
        if target is not None:
            nav["target_lane"] = target
        pid = np.zeros(1, abi.PID_DT)[0]
        pid["target_speed"] = NORMAL_SPEED
        # (the route rows go with the record: the device localises by the cached nav.road0 / road1, the oracle by the route's entries)
        rows.update(nav=nav, pid=pid, route_roads=t.route_roads, route_nodes=t.route_nodes, final_lane=t.final_lane)
        return rec, rows

    def case(self, name, items, about=()):
        """items [(slot, (shape record, rows))]"""
        bodies = [(slot, rec) for slot, (rec, _) in items]
        rows = {}
        for slot, (_, rw) in items:
            for k, v in rw.items():
                rows.setdefault(k, []).append((slot, v))
        assert len(set(s for s, _ in bodies)) == len(bodies) and all(0 < s for s, _ in bodies), name
        if any(s >= self.cap for s, _ in bodies):
            return None      # the capacity has no such slot: the family does without this case
        return Case(name, self.agent, bodies, rows, about)

    # -- lanes --
    def lanes_where(self, pred):
        out = [l for l in sorted(self.tmpl) if pred(l)]
        return [out[k] for k in self.rng.permutation(len(out))]

    def straight(self, l):
        return self.mr.objs[l].kind == 0

    def axis_aligned(self, l):
        r = self.mr.mt.lanes[l]
        return self.straight(l) and (abs(float(r["bx"])) == 1.0 or abs(float(r["by"])) == 1.0) and min(abs(float(r["bx"])), abs(float(r["by"]))) < 1e-12

    def env_of(self, case):
        """the case's env rows on the base env (an empty one without it): premises and sensitivity, before any launch"""
        if self.base_env is not None:
            env = {k: v.copy() for k, v in self.base_env.items()}
        else:
            env = dict(shape=np.zeros(self.cap, abi.SHAPE_DT), dyn=np.zeros(self.cap, abi.DYN_DT), nav=np.zeros(self.cap, abi.NAV_DT),
                       pid=np.zeros(self.cap, abi.PID_DT))
            env["shape"]["aux"] = -1
            env["nav"]["lane"] = env["nav"]["target_lane"] = -1
        env["shape"][0] = case.agent
        for slot, rec in case.bodies:
            env["shape"][slot] = rec
        for k, rows in case.rows.items():
            for slot, rec in rows:
                if k in env:
                    env[k][slot] = rec
        return env

    def holds(self, case):
        """the named case sits where its name says: every `about` entry against the float64 reference"""
        try:
            check_about(self.mr, self.env_of(case), case, self.idm_rand)
        except AssertionError:
            return False
        return True

    def first(self, name, lanes, make):
        """the first lane of `lanes` on which make(l) gives a case whose premises hold"""
        for l in lanes:
            c = make(l)
            if c is not None and self.holds(c):
                return [c]
        return []


def idm_rand_table(cap):
    """the idm_rand rows the tests upload for one env: every slot draws, in [0, 25) as the host scene's do"""
    return np.random.RandomState(41).randint(0, 25, size=(cap, abi.MD_IDM_RAND)).astype(np.int32)


def check_about(mr, env, case, idm_rand):
    """the premises of a named case from the float64 reference -> the results of its egos"""
    out = {}
    for ab in case.about:
        ego = ab["ego"]
        r = out.get(ego) or evaluate(mr, env, ego, idm_rand[ego])
        out[ego] = r
        assert r.decided, (case.name, ego, sorted(r.margins, key=lambda m: m[1])[:3])
        if "fail" in ab:
            assert (r.participant or r.plan["fail"]) == ab["fail"], (case.name, r.participant)
        if "n_cand" in ab:
            assert len(r.cand) == ab["n_cand"], (case.name, len(r.cand), ab["n_cand"])
        if "steer_lane" in ab:
            assert r.policy["steer_lane"] == ab["steer_lane"], (case.name, r.policy, ab["steer_lane"])
        for k in DISCRETE:
            if k in ab:
                assert getattr(r, k) == ab[k], (case.name, k, getattr(r, k), ab[k])
        if "bucket" in ab:
            i, side = ab["bucket"]
            got = r.fb[side][i]
            assert got == ab["winner"], (case.name, ab["bucket"], got, ab["winner"], r.fb)
            if "gap" in ab:
                assert abs(r.fb[side + "_d"][i] - ab["gap"]) < 0.05, (case.name, r.fb[side + "_d"][i], ab["gap"])
            if "gap_sign" in ab:
                assert r.fb[side + "_d"][i] * ab["gap_sign"] > 0.0, (case.name, r.fb)
            if "front_obj" in ab:
                assert r.policy["front_obj"] == ab["front_obj"], (case.name, r.policy)
            for tag in ab.get("variants", ()):
                assert (i, side, tag) in r.sens, (case.name, tag, sorted(r.sens))
                ds, da, disc = r.sens[(i, side, tag)]
                if ab["word"] == "steer":
                    assert ds >= SENS_FACTOR * TOL_STEER, (case.name, tag, ds)
                else:
                    assert da >= SENS_FACTOR * acc_tol(r.acc), (case.name, tag, da, r.acc)
    return out


EGO, S0 = 1, 35.0     # the ego's usual slot and longitudinal


def nearest_cases(b, curve=None, tag="nearest"):
    """two same-lane objects on each side of the ego, the nearer one in the higher slot"""
    out = []
    pred = (lambda l: b.straight(l)) if curve is None else (lambda l: not b.straight(l) and b.mr.objs[l].clockwise == curve)
    for side, sgn in (("front", 1.0), ("back", -1.0)):
        def make(l, side=side, sgn=sgn):
            L = b.mr.objs[l]
            s0 = S0 if curve is None else 0.42 * L.length      # (the middle of an arc is the d_start > d_end branch point)
            far, near = (20.0, 12.0) if curve is None else (min(0.4 * L.length, 20.0), min(0.2 * L.length, 10.0))
            if side == "front":
                items = [(EGO, b.mover(l, s0, speed=6.0)), (5, b.body("vehicle", l, s0 + far, speed=2.0)), (9, b.body("vehicle", l, s0 + near, speed=4.0))]
                return b.case("%s_front:%d" % (tag, l), items, [dict(ego=EGO, bucket=(1, "front"), winner=9, gap=near, word="acc", variants=("runner", "none"))])
            # a back gap shows on a side lane only: the ego overtakes (slow front, timer > 50) and the side lane's back decides
            left, right = b.mr.neighbours(l)
            if left < 0 and right < 0:
                return None
            sl, i = (left, 0) if left >= 0 else (right, 2)
            s_side = b.mr.project(sl, *b.pose(l, s0)[:2])[0]
            items = [(EGO, b.mover(l, s0, speed=6.0, timer=60)), (3, b.body("vehicle", l, s0 + 12.0 if curve is None else s0 + near, speed=2.0)),
                     (5, b.body("vehicle", sl, s_side - 25.0 if curve is None else s_side - far)),
                     (9, b.body("vehicle", sl, s_side - 8.0 if curve is None else s_side - near))]
            if right >= 0 and i == 0:      # keep the right lane out of it
                items.append((11, b.body("vehicle", right, b.mr.project(right, *b.pose(l, s0)[:2])[0] - 6.0)))
            return b.case("%s_back:%d" % (tag, l), items, [dict(ego=EGO, bucket=(i, "back"), winner=9, steer_lane=l, word="steer",
                                                                variants=("none", ) + (("runner", ) if curve is None else ()))])
        out += b.first("%s_%s" % (tag, side), b.lanes_where(pred), make)
    return out


def tie_cases(b, ref_lane_local):
    """two same-lane objects with bit-equal float32 gaps and different speeds at lateral +-1 m of a straight, axis-aligned lane: the
    lower slot wins.  ref_lane_local(l, x, y) -> the oracle's float32 longitudinal"""
    def make(l):
        items = [(EGO, b.mover(l, S0, speed=6.0)), (7, b.body("vehicle", l, S0 + 15.0, lat=1.0, speed=1.0)),
                 (4, b.body("vehicle", l, S0 + 15.0, lat=-1.0, speed=9.0))]
        g = [ref_lane_local(l, float(items[k][1][0]["cx"]), float(items[k][1][0]["cy"])) for k in (1, 2)]
        if np.float32(g[0]).tobytes() != np.float32(g[1]).tobytes():
            return None
        # (at rest both stand still: which of the two wins cannot show, only that one does)
        return b.case("tie:%d" % l, items, [dict(ego=EGO, bucket=(1, "front"), winner=4, word="acc", variants=("none", ) if b.rest else ("runner", "none"))])
    return b.first("tie", b.lanes_where(b.axis_aligned), make)


def window_cases(b):
    """front gaps of 29.5 and 30.5 m and of +-0.5 m about the ego; back gaps likewise, on a side lane of an overtaking ego"""
    out = []
    for tag, gap, win in (("front_29.5", 29.5, 5), ("front_30.5", 30.5, -1), ("front_0.5", 0.5, 5), ("front_-0.5", -0.5, -1)):
        def make(l, tag=tag, gap=gap, win=win):
            items = [(EGO, b.mover(l, S0, speed=6.0)), (5, b.body("cone", l, S0 + gap))]
            ab = dict(ego=EGO, bucket=(1, "front"), winner=win, word="acc", variants=("none", ) if win >= 0 else ())
            return b.case("window:%s:%d" % (tag, l), items, [ab])
        out += b.first(tag, b.lanes_where(b.straight), make)
    for tag, gap, win in (("back_29.5", -29.5, 5), ("back_30.5", -30.5, -1), ("back_0.5", -0.5, 5), ("back_-0.5", 0.5, -1)):
        def make(l, tag=tag, gap=gap, win=win):
            left, right = b.mr.neighbours(l)
            if left < 0:
                return None
            s_side = b.mr.project(left, *b.pose(l, S0)[:2])[0]
            items = [(EGO, b.mover(l, S0, speed=6.0, timer=60)), (3, b.body("vehicle", l, S0 + 12.0, speed=2.0)),
                     (5, b.body("cone", left, s_side + gap, lat=-1.0))]
            # 29.5 m behind does not keep the ego from changing (> 15 m), 0.5 m behind does; 0.5 m AHEAD is a front object at rest
            ab = dict(ego=EGO, bucket=(0, "back"), winner=win, word="steer", variants=("none", ) if abs(gap) < 15.0 and win >= 0 else ())
            return b.case("window:%s:%d" % (tag, l), items, [ab])
        out += b.first(tag, b.lanes_where(b.straight), make)
    return out


def connected_cases(b, curve=None, tag="connected"):
    """the ego within 10 m of its lane's end (start), the object on the successor (predecessor) lane: once alone, once with a
    same-lane object in that bucket, which keeps the connected one out"""
    out = []
    kind_ok = (lambda l: True) if curve is None else (lambda l: not b.straight(l) and b.mr.objs[l].clockwise == curve)
    for blocked in (False, True):
        def make_front(l, blocked=blocked):
            L = b.mr.objs[l]
            if not b.mr.succ[l] or L.length < 12.0:
                return None
            nl = b.mr.succ[l][0]
            s0 = L.length - 6.0
            items = [(EGO, b.mover(l, s0, speed=6.0)), (9, b.body("vehicle", nl, min(8.0, 0.5 * b.mr.objs[nl].length), speed=2.0))]
            if blocked:      # a same-lane front FARTHER away than the connected one still keeps it out
                items.append((12, b.body("cone", l, s0 + 20.0, lat=1.0)))
            ab = dict(ego=EGO, bucket=(1, "front"), winner=12 if blocked else 9, word="acc", variants=("none", ))
            return b.case("%s_front:%s:%d" % (tag, "blocked" if blocked else "alone", l), items, [ab])

        def make_back(l, blocked=blocked):
            # on the LEFT lane of an overtaking ego: the left lane's predecessor holds the object behind
            left, _ = b.mr.neighbours(l)
            if left < 0 or not b.mr.pred[left]:
                return None
            pl_ = b.mr.pred[left][0]
            P = b.mr.objs[pl_]
            s0 = 6.5      # (beyond the first 5 m of the lane, where a step's localiser moves the route cursors on)
            items = [(EGO, b.mover(l, s0, speed=6.0, timer=60)), (3, b.body("vehicle", l, s0 + 12.0, speed=2.0)),
                     (9, b.body("vehicle", pl_, P.length - min(4.0, 0.5 * P.length)))]
            if blocked:      # a same-lane back object 20 m behind (measured on the left lane, beyond its start): > 15 m, lets the ego change
                items.append((12, b.body("cone", left, b.mr.project(left, *b.pose(l, s0)[:2])[0] - 20.0, lat=1.0)))
            ab = dict(ego=EGO, bucket=(0, "back"), winner=12 if blocked else 9, word="steer", steer_lane=left if blocked else l,
                      variants=() if blocked else ("none", ))
            return b.case("%s_back:%s:%d" % (tag, "blocked" if blocked else "alone", l), items, [ab])
        lanes = b.lanes_where(lambda l: kind_ok(l))
        out += b.first("front", lanes, make_front) + b.first("back", lanes if curve is not None else b.lanes_where(b.straight), make_back)
    return out


def negative_back_cases(b):
    """objects whose aux names the predecessor of the overtaking ego's left lane but which stand BEYOND the ego: connected back
    gaps < 0, the more negative one in the higher slot, plus a positive one of 16.5 m in between: the smallest gap is the most negative
    one and keeps the ego on its lane, the positive one alone would let it change"""
    def make(l):
        left, _ = b.mr.neighbours(l)
        if left < 0 or not b.mr.pred[left] or not b.straight(b.mr.pred[left][0]):
            return None
        pl_ = b.mr.pred[left][0]
        P = b.mr.objs[pl_]
        s0 = 6.5
        cur = b.mr.project(left, *b.pose(l, s0)[:2])[0]
        at = lambda gap: P.length + cur - gap        # the longitudinal on the predecessor that gives this back gap
        # placed through the predecessor's own frame, extended beyond its end
        items = [(EGO, b.mover(l, s0, speed=6.0, timer=60)), (3, b.body("vehicle", l, s0 + 12.0, speed=2.0)),
                 (5, b.body("cone", pl_, at(-18.0), lat=1.0)), (9, b.body("cone", pl_, at(-24.0), lat=1.0)),
                 (7, b.body("cone", pl_, at(16.5), lat=1.0))]      # 16.5 m behind would let the ego change: the order across the sign shows
        ab = dict(ego=EGO, bucket=(0, "back"), winner=9, gap_sign=-1.0, steer_lane=l, word="steer", variants=("none", ))
        return b.case("negative_back:%d" % l, items, [ab])
    return b.first("negative_back", b.lanes_where(b.straight), make)


def side_gap_cases(b):
    """the overtake situation (ego and front more than 3 km/h off 30, timer > 50), the side lane empty but for one object 14 or 16 m
    behind: the steering lane flips with it.  An object 14 or 16 m AHEAD is a front object either way (its own speed decides, never
    the 15 m test); with a fast one the ego changes and takes it as the front object at that distance."""
    out = []
    for side in ("left", "right"):
        for tag, gap, speed in (("behind_14", -14.0, 0.0), ("behind_16", -16.0, 0.0), ("ahead_14", 14.0, 12.0), ("ahead_16", 16.0, 12.0)):
            def make(l, side=side, tag=tag, gap=gap, speed=speed):
                left, right = b.mr.neighbours(l)
                sl, i = (left, 0) if side == "left" else (right, 2)
                if sl < 0 or (side == "right" and left >= 0):       # the right lane is asked only when the left one offers nothing
                    return None
                s_side = b.mr.project(sl, *b.pose(l, S0)[:2])[0]
                items = [(EGO, b.mover(l, S0, speed=6.0, timer=60)), (3, b.body("vehicle", l, S0 + 12.0, speed=2.0)),
                         (9, b.body("vehicle", sl, s_side + gap, speed=speed))]
                # at rest the object ahead is no faster than the front: the ego stays, and would go without it
                changes = tag == "behind_16" or (gap > 0 and not b.rest)
                ab = dict(ego=EGO, bucket=(i, "back" if gap < 0 else "front"), winner=9, steer_lane=sl if changes else l,
                          word="acc" if changes and gap > 0 else "steer", variants=() if tag == "behind_16" else ("none", ))
                if changes:
                    ab["timer"] = 60
                return b.case("side_gaps:%s_%s:%d" % (side, tag, l), items, [ab])
            out += b.first(tag, b.lanes_where(b.straight), make)
    return out


def slot_cases(b):
    """one object in slot 63, 64 or 127 with the ego in a low slot; the ego itself in slot 63, 64 or 127; a not-alive, a kind-none and
    an aux = -1 body at the winning position change nothing"""
    out = []
    high = [s for s in (63, 64, 127) if s < b.cap]
    for s in high:
        def make(l, s=s):
            items = [(EGO, b.mover(l, S0, speed=6.0)), (s, b.body("vehicle", l, S0 + 14.0, speed=2.0))]
            return b.case("slots:object_%d:%d" % (s, l), items, [dict(ego=EGO, bucket=(1, "front"), winner=s, word="acc", variants=("none", ))])
        out += b.first("object", b.lanes_where(b.straight), make)

        def make_ego(l, s=s):
            items = [(s, b.mover(l, S0, speed=6.0)), (2, b.body("vehicle", l, S0 + 14.0, speed=2.0))]
            return b.case("slots:ego_%d:%d" % (s, l), items, [dict(ego=s, bucket=(1, "front"), winner=2, word="acc", variants=("none", ))])
        out += b.first("ego", b.lanes_where(b.straight), make_ego)

    def make_ghosts(l):
        items = [(EGO, b.mover(l, S0, speed=6.0)), (20, b.body("vehicle", l, S0 + 20.0, speed=2.0)),
                 (3, b.body("vehicle", l, S0 + 8.0, flags=abi.KIND_VEHICLE | STATIC)),                    # not alive
                 (high[-1], b.body("vehicle", l, S0 + 8.0, lat=0.5, flags=abi.KIND_NONE | ALIVE | STATIC)),      # kind none
                 (6, b.body("cone", l, S0 + 8.0, lat=-0.5, aux=-1))]                                       # on no lane
        return b.case("slots:ghosts:%d" % l, items, [dict(ego=EGO, bucket=(1, "front"), winner=20, gap=20.0, n_cand=2, word="acc", variants=("none", ))])
    return out + b.first("ghosts", b.lanes_where(b.straight), make_ghosts)


def obj_lane_cases(b):
    """a static vehicle whose aux says the ego's lane while a stale nav.lane says another; a moving vehicle the other way round"""
    def make(l):
        others = [k for k in sorted(b.tmpl) if k != l and b.mr.road_of[k] != b.mr.road_of[l]]
        if not others:
            return None
        rec, rows = b.body("vehicle", l, S0 + 10.0, speed=2.0)
        nav = b.tmpl[others[0]].nav.copy()
        rows["nav"] = nav                                   # stale: says lane others[0]
        mv = b.mover(l, S0 + 18.0, speed=5.0, aux=others[0])     # moving on l, a stale aux says others[0]
        far = b.body("vehicle", others[0], 5.0, aux=others[0])
        far[1]["nav"] = b.tmpl[l].nav.copy()                    # a static vehicle elsewhere whose stale nav.lane says l: never the ego's front
        items = [(EGO, b.mover(l, S0, speed=6.0)), (5, (rec, rows)), (9, mv), (12, far)]
        return b.case("obj_lane:%d" % l, items, [dict(ego=EGO, bucket=(1, "front"), winner=5, gap=10.0, word="acc", variants=("runner", "none")),
                                                 dict(ego=9)])

    def make_moving(l):
        others = [k for k in sorted(b.tmpl) if b.mr.road_of[k] != b.mr.road_of[l]]
        if not others:
            return None
        mv = b.mover(l, S0 + 10.0, speed=5.0, aux=others[0])
        st_ = b.body("vehicle", l, S0 + 5.0, aux=others[0], speed=2.0)      # nearer, but its aux names another lane
        return b.case("obj_lane:moving:%d" % l, [(EGO, b.mover(l, S0, speed=6.0)), (9, mv), (5, st_)],
                      [dict(ego=EGO, bucket=(1, "front"), winner=9, gap=10.0, word="acc", variants=("none", )), dict(ego=9)])
    lanes = b.lanes_where(b.straight)
    return b.first("static", lanes, make) + b.first("moving", lanes, make_moving)


def _filler(b, l, n, slots):
    """n cones on a ring of 40 m around the ego's pose on lane l, on no lane: candidates that decide nothing"""
    x, y, _ = b.pose(l, S0)
    out = []
    for k, s in enumerate(slots[:n]):
        a = 2.0 * math.pi * k / max(n, 1)
        rec = cr.make_shapes([x + 40.0 * math.cos(a)], [y + 40.0 * math.sin(a)], np.asarray([0.0]), 0.2, 0.2, BODIES["cone"][2])[0]
        rec["aux"] = -1
        out.append((s, (rec, {})))
    return out


def count_cases(b):
    """20, 21, 22, 23 and 70 candidates by the float64 ring test, none near the ring; the deciding objects hold the LAST ranks of the
    ascending slot order.  ring_21_22: 21 clear candidates and one body 0.3 m inside or outside the ring"""
    out = []

    def make(l, n, name, ring=None):
        slots = list(range(2, 2 + n + 4))
        fill = _filler(b, l, n - 2, slots)
        last = slots[n - 2], slots[n - 1]
        items = [(EGO, b.mover(l, S0, speed=6.0))] + fill + [(last[0], b.body("vehicle", l, S0 + 22.0, speed=2.0)),
                                                              (last[1], b.body("vehicle", l, S0 + 13.0, speed=4.0))]
        if ring is not None:      # a cone's rim `ring` metres inside (< 0: outside) the 50 m circle, straight ahead on the ego's lane, in slot 1 + ...
            items.append((b.cap - 8, b.body("cone", l, S0 + RING + 0.2 - ring, aux=-1)))
        ab = dict(ego=EGO, bucket=(1, "front"), winner=last[1], gap=13.0, n_cand=n + (ring is not None and ring > 0), word="acc",
                  variants=("runner", "none"))
        return b.case(name + ":%d" % l, items, [ab])
    for n in (20, 21, 22, 23, 70):
        out += b.first("count", b.lanes_where(b.straight), lambda l, n=n: make(l, n, "count_%d" % n))
    for tag, ring in (("in", 0.3), ("out", -0.3)):
        out += b.first("ring", b.lanes_where(b.straight), lambda l, tag=tag, ring=ring: make(l, 21, "ring_21_22:" + tag, ring))

    def make_connected(l, n):
        # the walks' second pass: the only front object stands on the successor lane, in the last rank (n = 70: the second chunk)
        L = b.mr.objs[l]
        if not b.mr.succ[l] or L.length < 12.0:
            return None
        nl, s0 = b.mr.succ[l][0], L.length - 6.0
        x, y, _ = b.pose(l, s0)
        fill = []
        for k in range(n - 1):
            a = 2.0 * math.pi * k / (n - 1)
            rec = cr.make_shapes([x + 40.0 * math.cos(a)], [y + 40.0 * math.sin(a)], np.asarray([0.0]), 0.2, 0.2, BODIES["cone"][2])[0]
            rec["aux"] = -1
            fill.append((2 + k, (rec, {})))
        items = [(EGO, b.mover(l, s0, speed=6.0))] + fill + [(1 + n, b.body("vehicle", nl, min(8.0, 0.5 * b.mr.objs[nl].length), speed=2.0))]
        ab = dict(ego=EGO, bucket=(1, "front"), winner=1 + n, n_cand=n, word="acc", variants=("none", ))
        return b.case("count_%d:connected:%d" % (n, l), items, [ab])
    for n in (22, 70):
        out += b.first("connected", b.lanes_where(lambda l: True), lambda l, n=n: make_connected(l, n))
    return out


def participant_cases(b):
    """a pedestrian (a circle) or a cyclist (an OBB) 0.3 m inside or outside the ring with a stopped vehicle 6 m ahead: inside, the
    fallback ignores the vehicle"""
    out = []
    for kind in ("pedestrian", "cyclist"):
        for tag, d in (("in", 0.3), ("out", -0.3)):
            def make(l, kind=kind, tag=tag, d=d):
                hl = BODIES[kind][0]
                items = [(EGO, b.mover(l, S0, speed=6.0)), (5, b.body("vehicle", l, S0 + 6.0)),
                         (9, b.body(kind, l, S0 - (RING + hl - d), aux=-1))]      # straight behind, its long axis along the lane
                ab = dict(ego=EGO, fail=tag == "in", bucket=(1, "front"), winner=5 if tag == "out" else -1)
                if tag == "out":
                    ab.update(word="acc", variants=("none", ))
                return b.case("participant_ring:%s_%s:%d" % (kind, tag, l), items, [ab])
            out += b.first(kind, b.lanes_where(b.straight), make)
    return out


def redraw_cases(b):
    """the ego stands on a lane of its road that is not its target lane: the target follows it and the timer is redrawn"""
    def make(l):
        left, right = b.mr.neighbours(l)
        other = left if left >= 0 else right
        if other < 0:
            return None
        items = [(EGO, b.mover(l, S0, speed=6.0, timer=7, target=other)), (5, b.body("vehicle", l, S0 + 14.0, speed=2.0))]
        want = int(b.idm_rand[EGO][0]) + 1
        return b.case("redraw:%d" % l, items, [dict(ego=EGO, target_lane=l, rand_cursor=1, timer=want)])
    return b.first("redraw", b.lanes_where(b.straight), make)


def forced_change_cases(b):
    """the ego outside the available lanes before a road with fewer lanes (lane_num_diff > 0): the side lane clear and blocked.  [] on
    a map without such a road.  (The side lane ABSENT -- md_idm_policy's fail path there -- cannot be placed from a nav record the
    engine produces: an index above the available lanes is above 0 and has a left lane on its road, one below them has a right
    lane; md_idm_plan scans both.)"""
    mr, out = b.mr, []

    def diff_of(l):
        nav = b.tmpl[l].nav
        if int(nav["ck1"]) == int(nav["ck0"]):
            return 0
        return int(mr.roads[int(nav["road0"])]["n_lanes"]) - int(mr.roads[int(nav["road1"])]["n_lanes"])
    for tag in ("clear", "blocked"):
        def make(l, tag=tag):
            nav = b.tmpl[l].nav
            cur, nxt = mr.roads[int(nav["road0"])], mr.roads[int(nav["road1"])]
            n, first = int(cur["n_lanes"]), int(cur["first_lane"])
            lo, hi = (0, int(nxt["n_lanes"]) - 1) if mr.prev[first, int(nxt["first_lane"])] else (diff_of(l), n - 1)
            i = mr.idx_of[l]
            if lo <= i <= hi:
                return None
            side, k = (l - 1, 0) if i > hi else (l + 1, 2)
            s0 = min(S0, 0.5 * mr.objs[l].length)
            items = [(EGO, b.mover(l, s0, speed=6.0))]
            if tag == "blocked":
                items.append((9, b.body("vehicle", side, mr.project(side, *b.pose(l, s0)[:2])[0] - 8.0)))
            ab = dict(ego=EGO, steer_lane=l if tag == "blocked" else side, target_speed=CREEP_SPEED if tag == "blocked" else NORMAL_SPEED)
            if tag == "blocked":
                ab.update(bucket=(k, "back"), winner=9, word="steer", variants=("none", ))
            return b.case("forced_change:%s:%d" % (tag, l), items, [ab])
        out += b.first(tag, b.lanes_where(lambda l: diff_of(l) > 0), make)
    return out


def fill_cases(b, n):
    """a random template lane, a random longitudinal and 0 ... 30 random bodies on the own, side and connected lanes"""
    out = []
    lanes = sorted(b.tmpl)
    kinds = ("vehicle", "cone", "warning", "barrier")
    rng = b.rng
    for k in range(n):
        l = lanes[rng.randint(0, len(lanes))]
        L = b.mr.objs[l]
        s0 = rng.uniform(1.0, L.length - 1.0)
        near = [x for x in (l, ) + b.mr.neighbours(l) if x >= 0]
        near += [y for x in list(near) for y in b.mr.succ[x] + b.mr.pred[x]]
        items = [(EGO, b.mover(l, s0, lat=rng.uniform(-0.5, 0.5), speed=rng.uniform(0.0, 12.0), timer=int(rng.randint(0, 80))))]
        pool = np.r_[2:12, 58:70, 120:128]
        slots = rng.permutation(pool[pool < b.cap - 1])[:rng.randint(0, 31)]
        for s in slots:
            ol = near[rng.randint(0, len(near))]
            OL = b.mr.objs[ol]
            so = rng.uniform(0.0, OL.length)
            at = np.asarray(b.pose(ol, so)[:2])
            if any(np.hypot(*(at - np.asarray([float(r["cx"]), float(r["cy"])]))) < 6.0 for _, (r, _) in items):
                continue      # bodies do not overlap: a front object a fraction of a metre ahead turns 1e-5 m of projection error into 1e-4 of the acceleration
            if ol in b.tmpl and rng.randint(0, 4) == 0:
                items.append((int(s), b.mover(ol, so, speed=rng.uniform(0.0, 12.0), timer=int(rng.randint(0, 80)))))
            else:
                items.append((int(s), b.body(kinds[rng.randint(0, len(kinds))], ol, so, lat=rng.uniform(-1.0, 1.0), speed=rng.uniform(0.0, 12.0))))
        if rng.randint(0, 8) == 0:
            items.append((b.cap - 1, b.body(("pedestrian", "cyclist")[rng.randint(0, 2)], l, s0 + rng.uniform(-60.0, 60.0), lat=3.0, aux=-1)))
        out.append(b.case("fill:%d" % k, items))
    return out


def group_cases(b):
    """four driving vehicles in a row on one lane, each the next one's back and the previous one's front: the one-wave-per-env
    kernel scans them one after the other through the same candidate list"""
    def make(l):
        if b.mr.objs[l].length < 40.0:
            return None
        items = [(k, b.mover(l, 4.0 + 9.0 * (k - 1), speed=3.0 + k, timer=10 * k)) for k in (1, 2, 3, 4)]
        items.append((70 if b.cap > 70 else 40, b.body("cone", l, 4.0 + 9.0 * 3 + 7.0)))
        about = [dict(ego=k, bucket=(1, "front"), winner=k + 1 if k < 4 else items[-1][0], word="acc", variants=("none", )) for k in (1, 2, 3, 4)]
        return b.case("group:%d" % l, items, about)
    return b.first("group", b.lanes_where(b.straight), make)


# The device test's launches, shared with the CPU test.  md_idm alone: (name, block sequence, staged: at most 64 lanes, curve families)
IDM_RUNS = [("staged_straight", "S$S", True, False), ("staged_curve", "C", True, True), ("nonstaged_intersection", "X", False, False),
            ("nonstaged_roundabout", "O", False, True), ("merge", "y", True, False)]
# one md_step from rest: (name, config, capacity) on STEP_MAP (more than 64 lanes: the lean kernels' non-staged forms)
STEP_MAP = "X"
STEP_RUNS = [("wg", dict(step_kernel="wg"), 128), ("narrow", dict(step_kernel="wg"), 64), ("wave", dict(step_kernel="wave"), 128),
             ("respawn", dict(traffic_mode="respawn", traffic_density=0.1), 128)]
IDM_FILL, STEP_FILL = 40, 24


def idm_run_cases(b, ref_long, curves):
    return named_cases(b, ref_long, curves=curves) + group_cases(b) + fill_cases(b, IDM_FILL)


def step_run_cases(b, ref_long):
    """the same families at rest; at capacity 64 without the cases that need a slot beyond 63 (slots 64 and 127, count_70)"""
    assert b.rest
    return named_cases(b, ref_long, small=b.cap <= 64) + group_cases(b) + fill_cases(b, STEP_FILL)


def clear_traffic(base, cap, A=1):
    """the traffic a config put into the base state, taken out: a placed env holds what its case placed and nothing else"""
    fl = base["shape"]["flags"].reshape(-1, cap)
    veh = ((fl & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((fl & STATIC) == 0)
    veh[:, :A] = False
    fl[veh] = 0
    base["action"].reshape(-1, cap, 2)[:, A:] = 0.0      # nor the action planned for it: a placed vehicle starts from rest and stays there
    return int(veh.sum())


WALK_FAMILIES = ("count_22", "count_23", "count_70")
PLACE_KEYS = ("shape", "dyn", "nav", "pid", "action", "flags", "route_roads", "route_nodes", "final_lane")
_COMMON = ("nearest_front", "nearest_back", "tie", "window", "connected_front", "connected_back", "negative_back", "side_gaps", "slots",
           "obj_lane", "count_20", "count_21", "count_22", "count_23", "ring_21_22", "participant_ring", "redraw", "group", "fill")
_CW, _CCW = ("curve_cw_front", "curve_cw_back"), ("curve_ccw_front", "curve_ccw_back")
# the families every launch set must hold (asserted before anything runs): a family a map cannot offer is asked of another one
NEEDED = {"staged_straight": _COMMON + ("count_70", ), "staged_curve": _COMMON + ("count_70", ) + _CW,
          "nonstaged_intersection": _COMMON + ("count_70", ), "nonstaged_roundabout": _COMMON + ("count_70", ) + _CW + _CCW,
          "merge": _COMMON + ("count_70", "forced_change"), "wg": _COMMON + ("count_70", ), "narrow": _COMMON, "wave": _COMMON + ("count_70", ),
          "respawn": _COMMON + ("count_70", )}
ALL_FAMILIES = _COMMON + ("count_70", "forced_change") + _CW + _CCW


def named_cases(b, ref_lane_local=None, curves=False, small=False):
    """every named family the map offers, then the walks' families again on their own (callers that want them alone filter)"""
    out = nearest_cases(b) + window_cases(b) + connected_cases(b) + negative_back_cases(b) + side_gap_cases(b) + slot_cases(b)
    out += obj_lane_cases(b) + count_cases(b) + participant_cases(b) + redraw_cases(b) + forced_change_cases(b)
    if ref_lane_local is not None:
        out += tie_cases(b, ref_lane_local)
    if curves:
        for cw, tag in ((True, "curve_cw"), (False, "curve_ccw")):
            out += nearest_cases(b, cw, tag) + connected_cases(b, cw, tag)
    if small:      # capacity 64: no slot beyond 63
        out = [c for c in out if all(s < b.cap for s, _ in c.bodies)]
        assert not any(c.family == "count_70" or c.name.startswith(("slots:object_64", "slots:object_127")) for c in out)
    return out


def families_of(cases):
    return set(c.family for c in cases)


# --------------------------------------------------------------------------------------------------
# placing, and checking a launch against the reference
# --------------------------------------------------------------------------------------------------
def place_rows(state, base, per_env, cap, keys=("shape", "dyn", "nav", "pid", "action", "flags")):
    """the host-side twin of the device rig's place(): restore the base, then one Case per env"""
    for k in keys:
        state[k][...] = base[k]
    for e, case in enumerate(per_env):
        for slot, rec in [(0, case.agent)] + case.bodies:
            state["shape"][e * cap + slot] = rec
            d = state["dyn"][e * cap + slot]
            d["heading"], d["speed"] = math.atan2(float(rec["s"]), float(rec["c"])), 0.0
            d["last_x"], d["last_y"], d["last_c"], d["last_s"] = rec["cx"], rec["cy"], rec["c"], rec["s"]
            state["dyn"][e * cap + slot] = d
        for k, rows in case.rows.items():
            for slot, rec in rows:
                state[k][e * cap + slot] = rec


class Tally:
    """what one test checked: driving vehicles, undecided ones, the largest gaps of the two action words on decided vehicles"""
    def __init__(self):
        self.launches = self.vehicles = self.undecided = self.named_undecided = self.moved = 0
        self.d_steer = self.d_acc = 0.0
        self.families = set()

    def finish(self, name):
        print("%s: %d launches, %d driving vehicles checked (%d more retired or moved by the step), %d undecided (%.2f %%, named cases %d), largest |got - float64| steering %.2e "
              "acceleration %.2e (relative to max(1, |acc|)); families: %s" % (
                  name, self.launches, self.vehicles, self.moved, self.undecided, 100.0 * self.undecided / max(1, self.vehicles), self.named_undecided,
                  self.d_steer, self.d_acc, " ".join(sorted(self.families))))
        assert self.undecided <= UNDECIDED_CAP * self.vehicles and self.named_undecided == 0, (name, self.undecided, self.vehicles)


IDM_FIELDS = ("target_lane", "timer", "rand_cursor")      # of MdNav: what the IDM itself reads AND writes (with the whole MdPid)


def check_env(mr, placed, got, e, cap, case, idm_rand, tally, where, after_step=False, gaps=None):
    """Every driving vehicle of env e: the float64 reference of the PLACED rows against the rows `got` after the launch.
    after_step: the launch was a whole md_step from rest, whose IDM plans the NEXT step and so runs after the step's localiser
    -- which rewrites nav.lane / ck0 / ck1 / road0 / road1 and retires a vehicle that stands on no lane -- and after the respawns.
    The reference then reads what the IDM does not write (shapes, dyn, those nav fields) from `got` and what it does write
    (nav.target_lane / timer / rand_cursor, the pid rows) from the placed rows, for the vehicles that were placed, still drive and
    stand where they were placed.  The rest of the step leaves all four discrete fields of such a vehicle alone, so all four are
    compared.  gaps: a list that collects (|d steering|, |d acc| / max(1, |acc|), case, slot) instead of asserting them."""
    env = env_rows(placed, e, cap)
    slots = driving_slots(env)
    if after_step:
        now = env_rows(got, e, cap)
        nav = now["nav"].copy()
        for k in IDM_FIELDS:
            nav[k] = env["nav"][k]
        same = lambda j: all(now["shape"][k][j] == env["shape"][k][j] for k in ("cx", "cy", "hl", "hw", "flags", "aux"))
        slots = [j for j in slots if same(j)]      # (the integrator rewrites (c, s) from the heading, a rounding apart)
        tally.moved += len(driving_slots(env)) - len(slots)
        env = dict(shape=now["shape"], dyn=now["dyn"], nav=nav, pid=env["pid"])
    named = set(ab["ego"] for ab in case.about)
    for j in slots:
        r = evaluate(mr, env, j, idm_rand[j], sensitivity=False)
        tally.vehicles += 1
        if not r.decided:
            tally.undecided += 1
            tally.named_undecided += j in named
            continue
        n = e * cap + j
        for k in DISCRETE:
            g = got["pid"]["target_speed"][n] if k == "target_speed" else got["nav"][k][n]
            assert float(g) == float(getattr(r, k)), "%s env %d (%s) slot %d: %s is %s, float64 says %s (margin %.2e)" % (
                where, e, case.name, j, k, g, getattr(r, k), r.margin)
        st, acc = (float(v) for v in got["action"].reshape(-1, 2)[n])
        ds, da = abs(st - r.steering), abs(acc - r.acc) / max(1.0, abs(r.acc))
        if gaps is not None:
            gaps.append((ds, da, case.name, j))
        else:
            assert ds <= TOL_STEER and da <= TOL_ACC, \
                "%s env %d (%s) slot %d: action (%.7g, %.7g), float64 (%.7g, %.7g), front %s at %.4f, steering lane %d, margin %.2e" % (
                    where, e, case.name, j, st, acc, r.steering, r.acc, r.policy["front_obj"], r.policy["front_dist"], r.policy["steer_lane"], r.margin)
        tally.d_steer, tally.d_acc = max(tally.d_steer, ds), max(tally.d_acc, da)
    tally.families.add(case.family)
