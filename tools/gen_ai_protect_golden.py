#!/usr/bin/env python
"""Generate tests/golden/ai_protect.npz: the reference's own AIProtectPolicy.act (policy/AI_protect_policy.py:8-61, with the
expert_takeover branch of ManualControlPolicy.act, policy/manual_control_policy.py:46-68) on stub objects.  TEST INFRASTRUCTURE.

Run where the reference tree is (it imports it through oracle/gen/refshim.py, read-only; nothing under oracle/ changes):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_ai_protect_golden.py

What is the reference's: AIProtectPolicy.act / ManualControlPolicy.act / EnvInputPolicy.act, the numpy expert (numpy_expert.expert
with `_expert_weights` = the npz of tests/golden and `_expert_observation` = a stub whose observe() returns the case's row, as
tools/gen_expert_golden.py sets them; the package picks the numpy expert where torch is absent, which is arranged for the import),
np.random.normal's draw (np.random seeded once), and BaseVehicle.heading_diff on real StraightLane / CircularLane objects of both
senses.  What is stubbed: a controller whose process_others does nothing (the reference calls it on None when manual_control is
False, manual_control_policy.py:44,48, so it cannot run this headless), an engine holding global_config, agent_manager (active_agents,
get_agent, observations[id].cloud_points), current_track_agent, main_camera = None and external_actions, and a vehicle with plain
attributes.

Every case stores all inputs (save_level, the agent's action, the observation row as pool row + its first three dims, the cloud,
the vehicle's lane record, pose, speeds, expert_takeover, the takeover state before the call), the sampled saver_a, the returned
action and action_info, and `margin`: the smallest relative distance |a - b| / max(|a|, |b|) of any quantity the saver compares
from its threshold (obs[0], obs[1] against 0.04 f and 1e-3, heading_diff against 0.5, the window minima against their limits).
The reference compares in float64 (or float32, as numpy's promotion has it), the device in float32: cases with margin <= 1e-5 are
left out by the tests, and at most 2 % of the cases may be such.  The tests of save_level against 0.9 and 1e-3, of the throttles
against 0 and of speed_km_h against 5 compare float32-representable inputs with constants that both precisions hold alike; they
carry no margin.  Chains are consecutive calls on one vehicle (chain >= 0, in order), so start / hold / end all occur.
"""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "gen")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import expert_host as eh  # noqa: E402

OUT = os.environ.get("MD_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
LEVELS = (0.0, 1e-3, 0.05, 0.3, 0.5, 0.9, 0.95, 1.0)
N_POOL = 32
NEAR = 1e-5


def f32(x):
    return float(np.float32(x))


def import_reference():
    import refshim
    refshim.install()
    real = importlib.util.find_spec
    importlib.util.find_spec = lambda name, *a, **k: None if name == "torch" else real(name, *a, **k)   # the numpy expert
    try:
        from metadrive.examples.ppo_expert import numpy_expert as ne
        import metadrive.examples.ppo_expert as pe
        assert pe.expert is ne.expert
        from metadrive.policy import base_policy
        from metadrive.policy.AI_protect_policy import AIProtectPolicy
    finally:
        importlib.util.find_spec = real
    from metadrive.component.lane.circular_lane import CircularLane
    from metadrive.component.lane.straight_lane import StraightLane
    from metadrive.component.vehicle.base_vehicle import BaseVehicle
    return ne, base_policy, AIProtectPolicy, StraightLane, CircularLane, BaseVehicle


def main():
    ne, base_policy, AIProtectPolicy, StraightLane, CircularLane, BaseVehicle = import_reference()
    rng = np.random.RandomState(20240)
    np.random.seed(777)

    # -- the expert as the reference's generator sets it ------------------------------------------------------------------
    class _ObsStub:
        row = None

        def observe(self, vehicle):
            return self.row.copy()

    obs_stub = _ObsStub()
    ne._expert_weights = dict(np.load(eh.WEIGHTS))
    ne._expert_observation = obs_stub
    # observation rows: the pool gives the MLP varied inputs (both signs of the saver's throttle); dims 0..2 are set per case
    pool = rng.uniform(0.0, 1.0, (N_POOL, 275)).astype(np.float32)
    pool[: N_POOL // 2, 19 + 16:] = 1.0          # a free road ahead ...
    pool[N_POOL // 2:, 19 + 16: 19 + 16 + 20] = rng.uniform(0.02, 0.2, (N_POOL - N_POOL // 2, 20)).astype(np.float32)   # ... or a wall
    pool[N_POOL // 2:, -20:] = pool[N_POOL // 2:, 19 + 16: 19 + 16 + 20]

    # -- lanes: the reference's objects and their MdLane fields -------------------------------------------------------------
    # (float32-representable geometry, so that the host restatement gets the reference's inputs exactly)
    lanes = [StraightLane([0, 0], [50, 0], 3.5), StraightLane([f32(3.2), -7.5], [f32(-40.1), f32(22.3)], 3.0)]
    for cw in (True, False):
        for radius, sp, ang in ((25.0, 0.3, 1.2), (60.0, -2.9, 2.3)):
            lanes.append(CircularLane((5.0, -3.0), radius, sp, ang, cw, 3.5))

    def lane_fields(lane):
        if isinstance(lane, StraightLane):
            return dict(type=0, sx=f32(lane.start[0]), sy=f32(lane.start[1]), ex=f32(lane.end[0]), ey=f32(lane.end[1]), ax=0.0, ay=0.0,
                        dirsign=0.0)
        return dict(type=1, sx=0.0, sy=0.0, ex=0.0, ey=0.0, ax=f32(lane.center[0]), ay=f32(lane.center[1]),
                    dirsign=-1.0 if lane.is_clockwise() else 1.0)

    # -- stubs -----------------------------------------------------------------------------------------------------------------
    class _Controller:
        def process_others(self, takeover_callback=None):
            return None

    def make_vehicle():
        v = SimpleNamespace(id="agent_vehicle", expert_takeover=False, takeover=False, config={"lidar": {"num_lasers": 240}},
                            max_speed_km_h=80.0)
        v.heading_diff = types.MethodType(BaseVehicle.heading_diff, v)
        return v

    veh_box = [make_vehicle()]
    observations = {"agent_vehicle": SimpleNamespace(cloud_points=None)}
    agent_manager = SimpleNamespace(active_agents={"default_agent": None}, observations=observations,
                                    get_agent=lambda agent_id: veh_box[0])
    engine = SimpleNamespace(global_config=dict(save_level=0.5, manual_control=False, action_check=False, discrete_action=False),
                             agent_manager=agent_manager, current_track_agent=None, main_camera=None, external_actions={})
    base_policy.get_engine = lambda: engine
    policy = object.__new__(AIProtectPolicy)
    policy.controller = _Controller()
    policy.enable_expert = True
    policy.action_info = {}
    policy.discrete_action = False

    cases = []

    def pose_for(lane, hd_side):
        """A pose on `lane` whose heading_diff is below (hd_side < 0) or above 0.5, at a random angle off the lane's direction"""
        s = float(rng.uniform(2.0, lane.length - 2.0))
        lat = float(rng.uniform(-1.5, 1.5))
        pos = lane.position(s, lat)
        # heading_diff = cos(heading, lateral direction) / 2 + 0.5: the sign of the off-lane angle decides the side; the sense
        # of it differs between lane kinds, so draw and let the reference say which side it is
        for _ in range(64):
            off = float(rng.uniform(0.02, 0.6)) * (1 if rng.rand() < 0.5 else -1)
            h = lane.heading_theta_at(s) + off
            v = SimpleNamespace(position=np.array([f32(pos[0]), f32(pos[1])]), heading=np.array([f32(np.cos(h)), f32(np.sin(h))]))
            hd = BaseVehicle.heading_diff(v, lane) - 0.5
            if hd_side == 0 or (hd < 0) == (hd_side < 0):
                return v.position, v.heading
        raise AssertionError("no pose")

    def run(veh, save_level, action, row_id, obs012, cloud, lane_id, pos, heading, speed, expert_takeover, chain, max_speed=80.0):
        lane = lanes[lane_id]
        row = pool[row_id].copy()
        row[0:3] = np.float32(obs012)
        obs_stub.row = row
        veh_box[0] = veh
        agent_manager.active_agents["default_agent"] = veh
        engine.current_track_agent = veh
        engine.global_config["save_level"] = save_level
        engine.external_actions = {"default_agent": [f32(action[0]), f32(action[1])]}
        cloud = np.asarray(cloud, np.float32)
        observations["agent_vehicle"].cloud_points = [float(c) for c in cloud]
        veh.lane, veh.position, veh.heading = lane, pos, heading
        veh.speed_km_h, veh.max_speed_km_h = f32(speed), f32(max_speed)
        veh.expert_takeover = bool(expert_takeover)
        pre = bool(veh.takeover)
        state = np.random.get_state()
        ret = policy.act("default_agent")
        info = dict(policy.action_info)
        # the draw the call made (one np.random.normal(mean, std) in either branch): replayed from the saved stream state
        np.random.set_state(state)
        obs_stub.row = row
        saver_a = ne.expert(SimpleNamespace(config={}), deterministic=False)
        hd = float(BaseVehicle.heading_diff(veh, lane))
        # margins of the compared quantities (float64 restatement of the saver's own expressions)
        margin = 1.0
        if not expert_takeover and 1e-3 < save_level <= 0.9:
            d = hd - 0.5
            f = min(1 + abs(d) * veh.speed_km_h * veh.max_speed_km_h, save_level * 10)
            lp = [float(c) for c in cloud]
            pairs = [(float(row[0]), 0.04 * f), (float(row[1]), 0.04 * f), (hd, 0.5), (float(row[0]), 1e-3), (float(row[1]), 1e-3),
                     (min(lp[56:66]), (save_level + 0.1) / 10), (min(lp[176:186]), (save_level + 0.1) / 10),
                     (min(min(lp[0:10]), min(lp[-10:])), save_level)]
            margin = min(abs(a - b) / max(abs(a), abs(b), 1e-30) for a, b in pairs)
        lf = lane_fields(lane)
        c = dict(save_level=save_level, action=[f32(action[0]), f32(action[1])], row_id=row_id, obs012=[float(x) for x in row[0:3]], cloud=cloud,
                 lane_id=lane_id, pos=[float(pos[0]), float(pos[1])], heading=[float(heading[0]), float(heading[1])],
                 speed_km_h=veh.speed_km_h, max_speed_km_h=veh.max_speed_km_h, expert_takeover=bool(expert_takeover), pre_takeover=pre,
                 chain=chain, heading_diff=hd, saver_a=[float(saver_a[0]), float(saver_a[1])], out_action=[float(ret[0]), float(ret[1])],
                 takeover_after=bool(veh.takeover), info_takeover=bool(info["takeover"]), info_start=bool(info["takeover_start"]),
                 info_end=bool(info["takeover_end"]), margin=float(margin), **{"lane_" + k: v for k, v in lf.items()})
        assert [float(x) for x in info["action"]] == c["out_action"]
        cases.append(c)
        return c

    def free_cloud():
        return np.ones(240, np.float32)

    def rand_action():
        return [float(rng.uniform(-1.3, 1.3)), float(rng.choice([0.0, 1.0, -1.0, float(rng.uniform(-1.3, 1.3))]))]

    def random_case(level, veh=None, chain=-1, pre=None, **over):
        lane_id = int(rng.randint(len(lanes)))
        pos, heading = pose_for(lanes[lane_id], 0)
        other = lanes[(lane_id + 1 + int(rng.randint(len(lanes) - 1))) % len(lanes)]      # obs dim 2 looks at ANOTHER lane
        hd_ref = BaseVehicle.heading_diff(SimpleNamespace(position=pos, heading=heading), other)
        cloud = free_cloud()
        k = rng.rand()
        if k < 0.5:          # a few obstacles anywhere
            idx = rng.randint(0, 240, int(rng.randint(1, 6)))
            cloud[idx] = rng.uniform(0.005, 0.6, len(idx)).astype(np.float32)
        kw = dict(save_level=level, action=rand_action(), row_id=int(rng.randint(N_POOL)),
                  obs012=[float(rng.choice([rng.uniform(0.0, 0.02), rng.uniform(0.02, 0.5)])),
                          float(rng.choice([rng.uniform(0.0, 0.02), rng.uniform(0.02, 0.5)])), float(hd_ref)],
                  cloud=cloud, lane_id=lane_id, pos=pos, heading=heading, speed=float(rng.choice([rng.uniform(0, 5), rng.uniform(5, 80)])),
                  expert_takeover=False, chain=chain)
        kw.update(over)
        if veh is None:      # a vehicle in either takeover state: the saver's action shows in the applied one only after a takeover step
            veh = make_vehicle()
            veh.takeover = bool(pre if pre is not None else rng.rand() < 0.5)
        return run(veh, **kw)

    # A. every save_level, random situations
    for level in LEVELS:
        for _ in range(26):
            random_case(level)
    # B. every clause of the out-of-road test alone, speed either side of 5
    for level in (0.05, 0.3, 0.5, 0.9):
        for clause in range(4):
            for speed in (3.0, 4.9990234375, 5.0, 30.0):
                lane_id = int(rng.randint(len(lanes)))
                # clause 0: obs0 < 0.04 f and hd < 0; 1: obs1 < 0.04 f and hd > 0; 2: obs0 <= 1e-3 (hd > 0); 3: obs1 <= 1e-3 (hd < 0)
                side = -1 if clause in (0, 3) else 1
                pos, heading = pose_for(lanes[lane_id], side)
                small = 0.0005 if clause >= 2 else 0.015
                o = [0.45, 0.45]
                o[clause % 2] = small
                random_case(level, lane_id=lane_id, pos=pos, heading=heading, obs012=[o[0], o[1], 0.5], cloud=free_cloud(), speed=speed, pre=True)
    # C. each lidar window alone: an obstacle at its first and last index, and just outside
    for level in (0.3, 0.5):
        for idxs in ((56, 65, 55, 66), (176, 185, 175, 186), (0, 9, 10), (230, 239, 229)):     # first, last, just outside
            for idx in idxs:
                for throttle in (1.0, 0.0, -0.5):
                    cloud = free_cloud()
                    cloud[idx] = np.float32(rng.uniform(0.004, 0.035))
                    lane_id = int(rng.randint(len(lanes)))
                    pos, heading = pose_for(lanes[lane_id], 0)
                    random_case(level, lane_id=lane_id, pos=pos, heading=heading, obs012=[0.45, 0.45, 0.5], cloud=cloud, speed=40.0,
                                action=[float(rng.uniform(-1, 1)), throttle], row_id=int(N_POOL // 2 + rng.randint(N_POOL // 2)), pre=True)
    # D. expert_takeover on, from both takeover states
    for level in (0.0, 0.5, 1.0):
        for pre in (False, True):
            for _ in range(6):
                v = make_vehicle()
                v.takeover = pre
                random_case(level, veh=v, expert_takeover=True)
    # E. chains on one vehicle: it drifts to the left edge heading out, is saved, and is let go again
    chain = 0
    for level in (0.05, 0.3, 0.5, 0.9, 1.0, 0.5, 0.3, 0.5):
        for _ in range(2):
            v = make_vehicle()
            lane_id = int(rng.randint(len(lanes)))
            profile = [0.31, 0.22, 0.012, 0.011, 0.010, 0.011, 0.22, 0.31, 0.012, 0.22, 0.31]
            for t, o0 in enumerate(profile):
                side = -1 if o0 < 0.1 else 1
                pos, heading = pose_for(lanes[lane_id], side)
                et = level == 0.5 and chain % 4 == 3 and t == 5
                random_case(level, veh=v, chain=chain, lane_id=lane_id, pos=pos, heading=heading, obs012=[o0, 0.45, 0.5], cloud=free_cloud(),
                            speed=float(rng.uniform(20, 60)), expert_takeover=et, action=[float(rng.uniform(-1, 1)), 1.0])
            chain += 1

    # -- coverage and the near-tie cap -----------------------------------------------------------------------------------
    n = len(cases)
    near = sum(c["margin"] <= NEAR for c in cases)
    assert near <= 0.02 * n, (near, n)
    kinds = set()
    for c in cases:
        kinds.add((c["info_takeover"], c["info_start"], c["info_end"]))
    assert {(False, True, False), (True, False, False), (False, False, True), (False, False, False)} <= kinds, kinds
    assert any(c["info_takeover"] and c["out_action"][1] == 0.5 for c in cases), "throttle = 0.5 below 5 km/h"
    assert any(c["info_takeover"] and c["out_action"][0] == c["action"][0] and c["out_action"][1] == c["saver_a"][1] for c in cases), \
        "the longitudinal test alone"
    assert any(c["info_takeover"] and c["out_action"][0] == c["saver_a"][0] and c["out_action"][1] == c["action"][1] for c in cases), \
        "the lateral test alone"
    assert any(abs(c["action"][0]) > 1 for c in cases)

    import refshim
    out = {}
    for k in cases[0]:
        v = [c[k] for c in cases]
        refshim.assert_plain(v, k)
        if k == "cloud":
            out[k] = np.asarray(v, np.float32)
        elif isinstance(cases[0][k], bool):
            out[k] = np.asarray(v, np.bool_)
        elif isinstance(cases[0][k], int):
            out[k] = np.asarray(v, np.int32)
        else:
            out[k] = np.asarray(v, np.float64)
    out["pool"] = pool
    path = os.path.join(OUT, "ai_protect.npz")
    np.savez_compressed(path, **out)
    print("wrote {} cases ({} within {:g} of a threshold), {} chains, {:.0f} KB".format(n, near, NEAR, chain, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
