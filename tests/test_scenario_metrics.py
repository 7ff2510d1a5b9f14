"""The closed-loop driving metrics of scenario mode (include/md_scenario_metrics.h) through its gcc host build
(tests/scenario_metrics_host.py): the sweep on placed states with answers worked out by hand, the finite differences bit for bit
against a float32 numpy restatement in the same operation order, the validity bits, the history rule, the accumulators and the latch
over scripted episodes, each comfort bound crossed alone, and a randomised check of the sweep and of the two wrapped columns against
float64."""
import math

import numpy as np
import pytest

import contact_ref as cr
import scenario_metrics_host as mh
from metadrive_ped_amd import abi

F = np.float32
S, E = mh.STEP, mh.EPISODE
NO_HIT_30 = F(F(30) * F(0.1)) + F(0.1)
OBSERVER_BITS = (1 << S("speed")) | (1 << S("ttc"))
FRAME_BITS = (1 << S("log_divergence")) | (1 << S("log_heading_error"))
RATE_BITS = (1 << S("lon_accel")) | (1 << S("yaw_rate")) | (1 << S("lat_accel"))
JERK_BITS = (1 << S("lon_jerk")) | (1 << S("yaw_accel")) | (1 << S("jerk"))


def ttc_of(j, dt=0.1):
    return F(F(j) * F(dt))


# -- the sweep on placed states: the ego at the origin, heading 0, 10 m/s, half length 2.25 ----------------------------------------------
def test_a_stopped_car_ahead():
    # a 4.5 m car centred 25.3 m ahead: the faces are 25.3 - 2.25 - 2.25 = 20.8 m apart, the ego covers 1 m per sample: j = 21
    o = mh.run_placed([(25.3, 0.0, 0.0, 0.0)])
    assert o["step"][S("ttc")] == ttc_of(21) and o["ttc_slot"] == 1 and o["step_valid"] & (1 << S("ttc"))
    assert o["step"][S("speed")] == 10.0 and o["step_valid"] == OBSERVER_BITS, "no frame put, no history, no lights"


def test_no_hit_within_the_samples_returns_the_sentinel():
    o = mh.run_placed([(40.0, 0.0, 0.0, 0.0)])      # 35.5 m between the faces, 30 samples reach 30 m
    assert o["step"][S("ttc")] == NO_HIT_30 and o["ttc_slot"] == -1 and o["step_valid"] & (1 << S("ttc")), "still a valid column"


def test_a_crossing_car_that_arrives_at_the_same_time():
    # from (20, -20) northwards at 10 m/s: both centres are at (20, 0) after 2 s.  The ego's front reaches the car's near side
    # (19.1) at 1.685 s, when the car's front reaches the ego's right side (-0.9) too: the first overlapping sample is j = 17
    o = mh.run_placed([(20.0, -20.0, 0.5 * math.pi, 10.0)])
    assert o["step"][S("ttc")] == ttc_of(17) and o["ttc_slot"] == 1


def test_a_diverging_car_never_hits():
    o = mh.run_placed([(5.0, 5.0, 0.5 * math.pi, 10.0)])
    assert o["step"][S("ttc")] == NO_HIT_30 and o["ttc_slot"] == -1
    o = mh.run_placed([(8.0, 0.0, 0.0, 10.0)])      # the same speed ahead: the gap stays
    assert o["step"][S("ttc")] == NO_HIT_30 and o["ttc_slot"] == -1
    o = mh.run_placed([(8.0, 0.0, 0.0, 5.0)])       # 3.5 m between the faces closing at 5 m/s: 0.7 s
    assert o["step"][S("ttc")] == ttc_of(7) and o["ttc_slot"] == 1


def test_the_lowest_slot_wins_a_tie_and_the_earlier_sample_beats_the_lower_slot():
    near, far, nearer = (25.3, 0.0, 0.0, 0.0), (40.0, 0.0, 0.0, 0.0), (14.8, 0.0, 0.0, 0.0)
    o = mh.run_placed([near, (25.3, 1.0, 0.0, 0.0)])
    assert o["step"][S("ttc")] == ttc_of(21) and o["ttc_slot"] == 1
    o = mh.run_placed([far, near, (25.3, -1.0, 0.0, 0.0)])
    assert o["step"][S("ttc")] == ttc_of(21) and o["ttc_slot"] == 2
    o = mh.run_placed([near, nearer])               # 10.3 m between the faces: j = 11
    assert o["step"][S("ttc")] == ttc_of(11) and o["ttc_slot"] == 2


def test_an_existing_overlap_is_sample_zero():
    o = mh.run_placed([(40.0, 0.0, 0.0, 0.0), (3.0, 0.5, 0.3, 4.0)])
    assert o["step"][S("ttc")] == 0.0 and o["ttc_slot"] == 2 and o["step_valid"] & (1 << S("ttc"))


def test_absent_movers_are_not_swept_and_circles_are_their_bounding_square():
    w, s, k, st = mh.metrics_world()
    mh.put_ego(st, 0.0, 0.0, 0.0, 10.0)
    mh.put(st, 1, 3.0, 0.0, flags=0)                                             # on the ego, but not alive
    mh.put(st, 2, 10.0, 0.0, kind=abi.KIND_PEDESTRIAN, hl=0.35, hw=0.35)          # 10 - 2.25 - 0.35 = 7.4 m: j = 8
    mh.put(st, 3, 6.0, 1.2, kind=abi.KIND_NONE)                                   # alive without a kind: not present
    o = mh.HostScenarioMetrics({}, 1).run(w, s, k).outputs()
    assert o["step"][0, S("ttc")] == ttc_of(8) and o["ttc_slot"][0] == 2
    # a pedestrian 1.2 m to the side of the path, 0.35 m radius: the square's corner (0.85) is inside the ego's side (0.9) ...
    o = mh.run_placed([(10.0, 1.2, 0.0, 0.0, 0.35, 0.35, abi.KIND_PEDESTRIAN)])
    assert o["step"][S("ttc")] == ttc_of(8)
    # ... and turned by 45 degrees the square reaches 0.35 * sqrt(2) = 0.495: 1.38 - 0.495 < 0.9 hits, 1.40 does not
    assert mh.run_placed([(10.0, 1.38, 0.25 * math.pi, 0.0, 0.35, 0.35, abi.KIND_PEDESTRIAN)])["ttc_slot"] == 1
    assert mh.run_placed([(10.0, 1.40, 0.25 * math.pi, 0.0, 0.35, 0.35, abi.KIND_PEDESTRIAN)])["ttc_slot"] == -1


def test_an_invalid_observer_makes_every_column_invalid():
    o = mh.run_placed([(3.0, 0.0, 0.0, 0.0)], present=False)
    assert not o["step"].any() and o["step_valid"] == 0 and o["ttc_slot"] == -1
    assert o["history"].view(np.int32)[5] == 0, "and leaves an empty history row"


def test_no_samples_but_the_first():
    o = mh.run_placed([(3.0, 0.0, 0.0, 0.0)], cfg=dict(ttc_samples=0))
    assert o["step"][S("ttc")] == 0.0 and o["ttc_slot"] == 1
    o = mh.run_placed([(6.0, 0.0, 0.0, 0.0)], cfg=dict(ttc_samples=0))
    assert o["step"][S("ttc")] == F(F(0) * F(0.1)) + F(0.1) and o["ttc_slot"] == -1
    o = mh.run_placed([(25.3, 0.0, 0.0, 0.0)], cfg=dict(ttc_samples=64, ttc_dt=0.25))      # 20.8 m at 2.5 m per sample: j = 9
    assert o["step"][S("ttc")] == ttc_of(9, 0.25) and o["ttc_slot"] == 1


# -- sequences fed step by step ------------------------------------------------------------------------------------------------------------
class Seq:
    """one env, the host build's rows kept from call to call"""
    def __init__(self, cfg=None, lights=False, T=16):
        self.w, self.s, self.k, self.st = mh.metrics_world(T=T)
        self.hm = mh.HostScenarioMetrics(cfg or {}, 1, lights=lights)

    def step(self, clock, v=0.0, h=0.0, x=0.0, y=0.0, flags=0, rc=0.0, present=True, light=0):
        mh.put_ego(self.st, x, y, h, v, clock=clock, flags=mh.EGO_FLAGS if present else 0)
        self.st["flags"][0], self.st["step_info"][0, 6], self.hm.agent_light[0] = flags, rc, light
        self.hm.run(self.w, self.s, self.k)
        return {n: a[0] for n, a in self.hm.outputs().items()}


DRIVE = [(0, 3.0, 0.10), (1, 3.4, 0.13), (2, 4.1, 0.11), (3, 4.0, 0.20)]        # (clock, speed, heading)


def test_finite_differences_bit_for_bit_and_the_validity_bits():
    q, D = Seq(), mh.step_period()
    rows = [q.step(t, v, h) for t, v, h in DRIVE]
    assert [int(r["step_valid"]) for r in rows] == [OBSERVER_BITS, OBSERVER_BITS | RATE_BITS, OBSERVER_BITS | RATE_BITS | JERK_BITS,
                                                    OBSERVER_BITS | RATE_BITS | JERK_BITS]
    assert not rows[0]["step"][3:9].any() and not rows[1]["step"][6:9].any(), "an invalid column holds 0"
    rates = [None] + [mh.rates_f32(DRIVE[i][1], DRIVE[i][2], DRIVE[i - 1][1], DRIVE[i - 1][2], D) for i in (1, 2, 3)]
    for i in (1, 2, 3):
        assert np.asarray(rates[i], F).tobytes() == rows[i]["step"][3:6].tobytes(), i
    for i in (2, 3):
        assert np.asarray(mh.jerks_f32(rates[i], rates[i - 1], D), F).tobytes() == rows[i]["step"][6:9].tobytes(), i
    assert rows[2]["step"][S("lon_accel")] == F(F(F(4.1) - F(3.4)) / D) and abs(rows[2]["step"][S("lon_accel")] - 7.0) < 1e-4
    assert abs(rows[2]["step"][S("yaw_rate")] + 0.2) < 1e-5 and abs(rows[2]["step"][S("lat_accel")] + 0.82) < 1e-4
    assert abs(rows[2]["step"][S("lon_jerk")] - 30.0) < 1e-3 and abs(rows[2]["step"][S("yaw_accel")] + 5.0) < 1e-3


def test_history_is_cleared_at_the_reset_and_by_a_clock_jump():
    q = Seq()
    for t, v, h in DRIVE:
        last = q.step(t, v, h)
    assert last["step_valid"] & JERK_BITS == JERK_BITS
    # a reset inside md_step: the clock is 0 again -- nothing to difference against, then one step later the rates, two the jerks
    r = [q.step(t, v, 0.0) for t, v in ((0, 1.0), (1, 1.5), (2, 1.5))]
    assert [int(x["step_valid"]) & (RATE_BITS | JERK_BITS) for x in r] == [0, RATE_BITS, RATE_BITS | JERK_BITS]
    assert r[1]["step"][S("lon_accel")] == F(F(F(1.5) - F(1.0)) / mh.step_period()), "against the reset state, not the old episode"
    # a clock jump (a restored checkpoint): the stored clock is not t - 1
    r = [q.step(t, 2.0, 0.0) for t in (7, 8, 9)]
    assert [int(x["step_valid"]) & (RATE_BITS | JERK_BITS) for x in r] == [0, RATE_BITS, RATE_BITS | JERK_BITS]
    # the same clock twice is no history either, and an invalid observer empties the row
    assert int(q.step(9, 2.0, 0.0)["step_valid"]) & RATE_BITS == 0
    q.step(10, 2.0, 0.0, present=False)
    assert int(q.step(11, 2.0, 0.0)["step_valid"]) & RATE_BITS == 0
    # zeroed rows (scenario_metrics_forget) at any clock
    q.step(12, 2.0, 0.0)
    q.hm.state[:] = 0
    assert int(q.step(13, 2.0, 0.0)["step_valid"]) & RATE_BITS == 0


def test_the_heading_wraps_across_pi():
    q, D = Seq(), mh.step_period()
    q.step(0, 5.0, 3.1)
    r = q.step(1, 5.0, -3.1)         # 0.0832 rad to the left, through pi
    want = F(mh.wrap_f32(F(F(-3.1) - F(3.1))) / D)
    assert r["step"][S("yaw_rate")] == want and abs(want - (2 * math.pi - 6.2) / 0.1) < 1e-4
    r = q.step(2, 5.0, 3.1)
    assert r["step"][S("yaw_rate")] == F(mh.wrap_f32(F(F(3.1) - F(-3.1))) / D) and r["step"][S("yaw_rate")] < 0


def test_divergence_and_heading_error_against_the_sdc_s_frame():
    q = Seq(T=4)
    mh.put_frame(q.st, 0, 0.0, 0.0, 0.0)
    mh.put_frame(q.st, 1, 3.0, 4.0, 3.0)
    mh.put_frame(q.st, 2, 1.0, 1.0, 0.0, flags=0)
    r = q.step(0, 0.0, 0.0)
    assert r["step_valid"] & FRAME_BITS == FRAME_BITS and r["step"][0] == 0.0 and r["step"][1] == 0.0
    r = q.step(1, 0.0, -3.0)
    assert r["step"][0] == 5.0 and r["step"][1] == abs(mh.wrap_f32(F(F(-3.0) - F(3.0)))) and abs(r["step"][1] - (2 * math.pi - 6)) < 1e-6
    assert not q.step(2, 0.0, 0.0)["step_valid"] & FRAME_BITS, "the record is not present"
    r = q.step(4, 0.0, 0.0, x=9.0)
    assert not r["step_valid"] & FRAME_BITS and r["step"][0] == 0.0, "past the scenario's frames"


def test_on_red_needs_the_lights():
    q = Seq(lights=True)
    r = q.step(1, light=abi.TL_BIT_RED | abi.TL_BIT_GREEN)
    assert r["step"][S("on_red")] == 1.0 and r["step_valid"] & (1 << S("on_red"))
    r = q.step(2, light=abi.TL_BIT_GREEN | abi.TL_BIT_YELLOW)
    assert r["step"][S("on_red")] == 0.0 and r["step_valid"] & (1 << S("on_red"))
    assert r["episode"][E("red_light_steps")] == 1.0
    r = Seq().step(1, light=abi.TL_BIT_RED)
    assert r["step"][S("on_red")] == 0.0 and not r["step_valid"] & (1 << S("on_red")) and not r["step_valid"] & (1 << 11)


# -- the accumulators and the latch ------------------------------------------------------------------------------------------------------
def test_accumulators_and_latch_over_two_episodes():
    q = Seq(lights=True, T=16)
    for t in range(8):
        mh.put_frame(q.st, t, 10.0 * t, 0.0, 0.0, flags=0 if t == 3 else mh.EGO_FLAGS)       # frame 3 is not valid
    w, s, k, st = q.w, q.s, q.k, q.st
    mh.put(st, 1, 1000.0, 0.0)      # a stopped car the ego closes in on during the first episode
    TR, TE, CR, OUT, ARR = abi.FL_TRUNCATED, abi.FL_TERMINATED, abi.FL_CRASH_VEHICLE, abi.FL_OUT_OF_ROAD, abi.FL_ARRIVE_DEST
    r0 = q.step(0, 10.0, 0.0, x=0.0)
    assert not r0["episode"][:5].any() and r0["episode"][E("min_ttc")] == NO_HIT_30 and not r0["episode"][6:].any()
    off = [None, 1.0, 3.0, 7.0, 2.0, 0.5, 4.0]          # the ego's lateral offset from the recorded drive at the steps 1 .. 6
    script = [None, dict(v=10.0), dict(v=10.5, light=4), dict(v=10.5, flags=CR), dict(v=10.0, flags=OUT, light=4),
              dict(v=10.0, flags=CR | OUT), dict(v=10.0, flags=TE | ARR, rc=0.875)]
    for t in range(1, 7):
        if t == 5:
            mh.put(st, 1, 10.0 * t + 4.6, off[t])        # 0.1 m between the faces: the first overlap is sample 1
        r = q.step(t, h=0.0, x=10.0 * t, y=off[t], **script[t])
    ep = r["episode"]
    assert ep[E("steps")] == 6
    valid = [off[t] for t in (1, 2, 4, 5, 6)]
    total = F(0)
    for d in valid:
        total = F(total + F(d))
    assert ep[E("ade")] == F(total / F(5)) and ep[E("max_divergence")] == 4.0 and ep[E("fde")] == 4.0, "step 3 has no frame"
    assert ep[E("max_heading_error")] == 0.0
    assert ep[E("min_ttc")] == ttc_of(1) and ep[E("ttc_violation_steps")] == 1
    assert ep[E("max_lon_accel")] == F(F(F(10.5) - F(10.0)) / mh.step_period()) and ep[E("min_lon_accel")] == F(F(F(10.0) - F(10.5)) / mh.step_period())
    assert ep[E("comfort_violation_steps")] == 4, "+5 m/s^2 at step 2 and -5 at step 4; jerks of 50, -50, -50, 50 m/s^3 at the steps 2 .. 5"
    assert ep[E("red_light_steps")] == 2 and ep[E("collision_steps")] == 2 and ep[E("out_of_road_steps")] == 2
    assert ep[E("route_completion")] == F(0.875) and ep[E("arrive_dest")] == 1 and not ep[20:].any()
    assert r["episodes"] == 1 and r["last_episode"].tobytes() == ep.tobytes()
    assert r["history"].view(np.int32)[7] == 1, "latched"
    first = r["last_episode"].copy()
    # the env stays on its last frame for one more launch (no auto-reset): no second latch
    r = q.step(7, 10.0, 0.0, x=70.0, flags=TE)
    assert r["episodes"] == 1 and r["last_episode"].tobytes() == first.tobytes() and r["episode"][E("steps")] == 7
    # the reset: the accumulators are emptied, the report stays
    mh.put(st, 1, 1000.0, 0.0)
    r = q.step(0, 0.0, 0.0)
    assert not r["episode"][:5].any() and r["episode"][E("min_ttc")] == NO_HIT_30 and not r["episode"][6:].any()
    assert r["episodes"] == 1 and r["last_episode"].tobytes() == first.tobytes() and r["history"].view(np.int32)[7] == 0
    for t in (1, 2):
        r = q.step(t, 1.0 * t, 0.0, x=10.0 * t, rc=0.25 * t, flags=TR if t == 2 else 0)
    assert r["episodes"] == 2 and r["last_episode"][E("steps")] == 2 and r["last_episode"][E("route_completion")] == 0.5
    assert r["last_episode"][E("arrive_dest")] == 0 and r["last_episode"][E("collision_steps")] == 0
    assert r["last_episode"][E("ade")] == 0.0 and r["last_episode"][E("min_ttc")] == NO_HIT_30
    assert r["last_episode"][E("max_lon_accel")] == F(F(1.0) / mh.step_period()) and r["last_episode"][E("min_lon_accel")] == 0.0
    r = q.step(0, 0.0, 0.0)
    assert r["episodes"] == 2 and r["last_episode"][E("steps")] == 2, "the report lasts until the env finishes another episode"


def test_an_absent_observer_adds_nothing_but_the_episode_still_latches():
    q = Seq()
    q.step(0, 1.0)
    q.step(1, 1.0)
    r = q.step(2, 1.0, present=False, flags=abi.FL_TRUNCATED)
    assert r["episode"][E("steps")] == 1 and r["episodes"] == 1 and r["last_episode"][E("steps")] == 1


# -- each comfort bound crossed alone ------------------------------------------------------------------------------------------------------
COMFORT = {       # name -> the (speed, heading) of the steps 0, 1[, 2]; worked out for D = 0.1 s
    "calm": [(5.0, 0.0), (5.1, 0.01), (5.2, 0.02)],
    "max_lon_accel": [(0.0, 0.0), (0.3, 0.0)],                    # 3 m/s^2 > 2.40
    "min_lon_accel": [(5.0, 0.0), (4.5, 0.0)],                    # -5 m/s^2 < -4.05
    "max_lat_accel": [(10.0, 0.0), (10.0, 0.05)],                 # 0.5 rad/s at 10 m/s: 5 m/s^2 > 4.89
    "max_yaw_rate": [(1.0, 0.0), (1.0, -0.1)],                    # -1 rad/s, |.| > 0.95; 1 m/s^2 sideways
    "max_lon_jerk": [(0.0, 0.0), (0.1, 0.0), (0.25, 0.0)],        # 1 then 1.5 m/s^2: 5 m/s^3 > 4.13, and a jerk of 5 < 8.37
    "max_jerk": [(10.0, 0.0), (10.0, 0.0), (10.0, 0.009)],        # 0.09 rad/s at 10 m/s: 0.9 m/s^2 in one step, 9 m/s^3 > 8.37
    "max_yaw_accel": [(1.0, 0.0), (1.0, 0.0), (1.0, 0.02)],       # 0 then 0.2 rad/s: 2 rad/s^2 > 1.93; 2 m/s^3 of jerk
}


@pytest.mark.parametrize("name", sorted(COMFORT))
def test_each_comfort_bound_crossed_alone(name):
    q, c = Seq(), mh.HostScenarioMetrics({}, 1).cfg
    for t, (v, h) in enumerate(COMFORT[name]):
        r = q.step(t, v, h)
    col, ok = r["step"], int(r["step_valid"])
    crossed = {"max_lon_accel": col[3] > c["max_lon_accel"], "min_lon_accel": col[3] < c["min_lon_accel"],
               "max_lat_accel": abs(col[5]) > c["max_lat_accel"], "max_yaw_rate": abs(col[4]) > c["max_yaw_rate"],
               "max_lon_jerk": bool(ok & (1 << 6)) and abs(col[6]) > c["max_lon_jerk"], "max_jerk": bool(ok & (1 << 8)) and col[8] > c["max_jerk"],
               "max_yaw_accel": bool(ok & (1 << 7)) and abs(col[7]) > c["max_yaw_accel"]}
    assert sorted(k for k, v in crossed.items() if v) == ([] if name == "calm" else [name])
    assert r["episode"][E("comfort_violation_steps")] == (0 if name == "calm" else 1)
    # the bound itself is not a violation: the same drive with the bound raised to the value reached
    if name != "calm":
        reached = {"max_lon_accel": col[3], "min_lon_accel": col[3], "max_lat_accel": abs(col[5]), "max_yaw_rate": abs(col[4]),
                   "max_lon_jerk": abs(col[6]), "max_jerk": col[8], "max_yaw_accel": abs(col[7])}[name]
        q = Seq({name: float(reached)})
        for t, (v, h) in enumerate(COMFORT[name]):
            r = q.step(t, v, h)
        assert r["episode"][E("comfort_violation_steps")] == 0


# -- randomised: the sweep and the two wrapped columns against float64 -------------------------------------------------------------------
N_CASES, N_MOVERS, SEED = 400, 3, 20


def _random_worlds():
    rng = np.random.RandomState(SEED)
    cases = []
    for _ in range(N_CASES):
        ego = (rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-math.pi, math.pi), rng.uniform(0, 15))
        movers = []
        for i in range(N_MOVERS):
            r, a = rng.uniform(4, 45), rng.uniform(-math.pi, math.pi)
            h, v = rng.uniform(-math.pi, math.pi), rng.uniform(-2, 15)
            if i == 2:       # the last mover drives ahead of the ego, roughly its way and slower: most of the hits
                a, h, v = ego[2] + rng.uniform(-0.1, 0.1), ego[2] + rng.uniform(-0.5, 0.5), rng.uniform(-2, 1) + 0.5 * ego[3]
            movers.append((ego[0] + r * math.cos(a), ego[1] + r * math.sin(a), h, v, rng.uniform(0.3, 3.0), rng.uniform(0.3, 1.2)))
        cases.append((ego, movers))
    return cases


def test_the_sweep_against_float64():
    """Decided cases must match exactly; a case is undecided when the ego grown and shrunk by contact_ref.EPS disagree at the deciding
    sample (the first pair, in key order, at which the grown ego overlaps); at most 2 % of the cases may be.  The placement ranges
    (movers 4 .. 45 m away, closing by up to a few metres per sample) make a 1 mm window at the deciding sample rare: with this seed the
    float64 reference alone leaves none of the 400 cases undecided (116 of them hit)."""
    J, dt = 30, 0.1
    cases = _random_worlds()
    undecided = hits = 0
    for ego, movers in cases:
        got = mh.run_placed([m for m in movers], ego=ego)
        # positions in float64 from the float32 inputs, one record per (sample, mover) in key order
        f = lambda v: float(F(v))
        recsA, recsB = [], []
        ce, se = float(F(math.cos(ego[2]))), float(F(math.sin(ego[2])))
        for j in range(J + 1):
            t = j * f(dt)
            for (x, y, h, v, hl, hw) in movers:
                c, s = float(F(math.cos(h))), float(F(math.sin(h)))
                recsA.append((f(ego[0]) + t * f(ego[3]) * ce, f(ego[1]) + t * f(ego[3]) * se, ce, se, f(mh.EGO_HL), f(mh.EGO_HW)))
                recsB.append((f(x) + t * f(v) * c, f(y) + t * f(v) * s, c, s, f(hl), f(hw)))
        dt64 = np.dtype([(k, np.float64) for k in ("cx", "cy", "c", "s", "hl", "hw")])
        A, B = np.array(recsA, dt64), np.array(recsB, dt64)
        big, same = cr.obb_obb(A, B)
        first = int(np.argmax(big)) if big.any() else -1
        if first >= 0 and not same[first]:
            undecided += 1
            continue
        if first < 0:
            assert got["ttc_slot"] == -1 and got["step"][S("ttc")] == NO_HIT_30, (ego, movers)
        else:
            j, n = divmod(first, N_MOVERS)
            hits += 1
            assert got["ttc_slot"] == 1 + n and got["step"][S("ttc")] == ttc_of(j), (ego, movers, j, n, got["ttc_slot"], got["step"][S("ttc")])
    print("undecided %d of %d, hits %d" % (undecided, N_CASES, hits))
    assert undecided <= 0.02 * N_CASES
    assert hits >= N_CASES // 5, "the case cannot pass empty"


def test_the_wrapped_columns_against_float64():
    """Columns 1 and 4 pass through md_wrap_to_pi, whose float32 result differs from the real one by the rounding of its operations on
    operands below 16 in magnitude (headings in [-2 pi, 2 pi], their difference below 4 pi):
      the difference h - h'               half an ulp of [8, 16)          2^-21 = 4.8e-7
      2 pi as a float32, times k, |k| <= 2  2 * |float32(2 pi) - 2 pi|   3.5e-7  (the product by 1 or 2 is exact)
      x - 2 pi k                          half an ulp of [4, 8)           2^-22 = 2.4e-7
      one guard's +- 2 pi                 the constant's error and half an ulp of [4, 8)   1.75e-7 + 2.4e-7
    together 1.5e-6 = 6.3 ulp of pi (2^-22 = 2.38e-7): the bound is 8 ulp of pi.  Column 4 divides by D once: 8 ulp of pi / D plus the
    division's own half ulp, 2^-24 of the quotient.  D enters the float64 reference as the float32 the header computes.  A pair of
    headings whose difference lies within the bound of the seam may wrap to the other side: column 4 is compared modulo 2 pi / D."""
    rng = np.random.RandomState(SEED + 1)
    bound, D = 8 * 2.0 ** -22, float(mh.step_period())
    seam = 0
    for i in range(300):
        h0, h1, hf = rng.uniform(-2 * math.pi, 2 * math.pi, 3)
        if i % 10 == 0:      # at the seam
            h1 = h0 + math.pi * rng.choice([-1, 1]) + rng.uniform(-1e-6, 1e-6)
            hf = h1 + math.pi
            seam += 1
        q = Seq(T=4)
        mh.put_frame(q.st, 1, 0.0, 0.0, hf)
        q.step(0, 1.0, h0)
        r = q.step(1, 1.0, h1)
        f0, f1, ff = float(F(h0)), float(F(h1)), float(q.st["track_dyn"][1, 0, 0])
        wrap = lambda x: math.pi - ((math.pi - x) % (2 * math.pi))          # to (-pi, pi]
        assert abs(float(r["step"][1]) - abs(wrap(f1 - ff))) <= bound, (h1, hf)
        want = wrap(f1 - f0) / D
        err = (float(r["step"][4]) - want + math.pi / D) % (2 * math.pi / D) - math.pi / D
        assert abs(err) <= bound / D + 2.0 ** -24 * abs(want), (h0, h1, float(r["step"][4]), want)
    assert seam == 30
