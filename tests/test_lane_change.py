"""agent_policy = LaneChangePolicy (policy/lange_change_policy.py) without a GPU: config, action spaces and decoding, the
refusals, the decide function (include/md_lane_change.h, host build) against a plain restatement of steering_control, and
the reference's known answer (tests/test_policy/test_lane_change_policy.py) on the CPU oracle driven by the host
restatement (tests/lane_change_host.py)."""
import ctypes as C

import numpy as np
import pytest

import lane_change_host as lh
from metadrive_ped_amd import abi

SINGLE = ("BatchedMetaDriveEnv", "BatchedSafeMetaDriveEnv", "BatchedVaryingDynamicsEnv")
MULTI = ("BatchedMultiAgentRoundaboutEnv", "BatchedMultiAgentIntersectionEnv", "BatchedMultiAgentTinyInter",
         "BatchedMultiAgentRacingEnv", "BatchedMultiAgentBottleneckEnv", "BatchedMultiAgentBidirectionEnv",
         "BatchedMultiAgentTollgateEnv", "BatchedMultiAgentParkingLotEnv", "BatchedMultiAgentMetaDrive")


def _env_class(name):
    import metadrive_ped_amd.envs as envs
    return getattr(envs, name)


@pytest.mark.parametrize("name", SINGLE + MULTI)
@pytest.mark.parametrize("multi_discrete", [False, True])
def test_action_space_is_three_by_throttle(name, multi_discrete):
    env = _env_class(name)(dict(agent_policy="LaneChangePolicy", discrete_action=True, use_multi_discrete=multi_discrete,
                                discrete_steering_dim=7, discrete_throttle_dim=4))
    sp = env.action_space
    if multi_discrete:
        assert list(sp.nvec) == [3, 4]
    else:
        assert sp.n == 12                      # 3 * throttle dim: discrete_steering_dim is ignored


def test_policy_class_of_that_name_is_accepted():
    from metadrive_ped_amd.config import make_config

    class LaneChangePolicy:
        pass

    cfg = make_config(dict(agent_policy=LaneChangePolicy, discrete_action=True))
    assert cfg["agent_policy"] == "LaneChangePolicy"


def test_decoding_discrete():
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.envs.metadrive_env import discrete_to_continuous
    cfg = make_config(dict(agent_policy="LaneChangePolicy", discrete_action=True, discrete_steering_dim=5, discrete_throttle_dim=5,
                           action_check=True))
    a = discrete_to_continuous(torch, cfg, torch.arange(15), (15, ), "cpu").numpy()
    idx = np.arange(15)
    assert np.array_equal(a[:, 0], (idx % 3 - 1).astype(np.float32))          # exactly -1, 0, +1
    assert np.array_equal(a[:, 1], ((idx // 3) * 0.5 - 1.0).astype(np.float32))
    with pytest.raises(AssertionError, match="not compatible"):
        discrete_to_continuous(torch, cfg, torch.tensor([15]), (1, ), "cpu")


def test_decoding_multi_discrete():
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.envs.metadrive_env import discrete_to_continuous
    cfg = make_config(dict(agent_policy="LaneChangePolicy", discrete_action=True, use_multi_discrete=True, discrete_steering_dim=5,
                           discrete_throttle_dim=5, action_check=True))
    a = discrete_to_continuous(torch, cfg, torch.tensor([[0, 0], [1, 2], [2, 4]]), (3, ), "cpu").numpy()
    assert np.array_equal(a, np.array([[-1, -1], [0, 0], [1, 1]], np.float32))
    with pytest.raises(AssertionError, match="not compatible"):      # steering 3 exists under discrete_steering_dim=5, not here
        discrete_to_continuous(torch, cfg, torch.tensor([[3, 0]]), (1, ), "cpu")


def test_other_policies_keep_their_spaces():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(discrete_action=True, discrete_steering_dim=7, discrete_throttle_dim=4))
    assert env.action_space.n == 28


def test_refuses_continuous_actions():
    from metadrive_ped_amd.config import make_config
    with pytest.raises(AssertionError, match="Must set discrete_action=True for using this control policy"):
        make_config(dict(agent_policy="LaneChangePolicy"))
    with pytest.raises(AssertionError, match="Must set discrete_action=True"):
        _env_class("BatchedMultiAgentRoundaboutEnv")(dict(agent_policy="LaneChangePolicy"))


def test_refused_in_scenario_env():
    from metadrive_ped_amd.scenario import make_scenario_config
    with pytest.raises(NotImplementedError, match="LaneChangePolicy"):
        make_scenario_config(dict(agent_policy="LaneChangePolicy", discrete_action=True))


def test_engine_config_field():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(make_config(dict(lh.CXO_CONFIG, num_envs=1, build_workers=1)))
    assert host.md_config.agent_idm == abi.AGENT_LANE_CHANGE
    host = HostScene(make_config(dict(map="CXO", num_envs=1, build_workers=1)))
    assert host.md_config.agent_idm == abi.AGENT_INPUT


def test_md_step_refuses_the_contradictions():
    """Scenario mode, and agent_idm values that name no policy (md_step's checks, called with dummy pointers: only where no
    GPU is visible, as tests/test_abi_requirements.py; tests/test_gpu_lane_change.py checks the same on real state)."""
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the calls use dummy pointers")
    import __graft_entry__ as g
    import abi_corpus
    lib = abi_corpus.open_lib(g.build_hip())
    decl = abi_corpus.declarations()["md_step"]
    buf = C.create_string_buffer(4096)
    dummy = (C.addressof(buf) + 15) & ~15
    rc, msg = abi_corpus._call(lib, "md_step", decl, dict(config=dict(abi_corpus.SCENE, agent_idm=2)), dummy, set())
    assert rc == abi.MD_EINVAL and "LaneChangePolicy" in msg and "scenario mode" in msg
    for v in (3, -1):
        rc, msg = abi_corpus._call(lib, "md_step", decl, dict(config=dict(agent_idm=v)), dummy, set())
        assert rc == abi.MD_EINVAL and msg.startswith("agent_idm=%d" % v)
    # the single- and multi-agent configs with the policy get past the checks (to the launch, which fails without a GPU)
    assert abi_corpus._call(lib, "md_step", decl, dict(config=dict(agent_idm=2)), dummy, set()) == "passed"
    assert abi_corpus._call(lib, "md_step", decl, dict(config=dict(abi_corpus.MULTI, agent_idm=2)), dummy, set()) == "passed"


# ---- the decide function ---------------------------------------------------------------------------------------------
class _Pid:
    """PIDController (component/vehicle/PID_controller.py), in float32 like the MdPid rows"""

    def __init__(self, kp, ki, kd):
        self.k = [np.float32(kp), np.float32(ki), np.float32(kd)]
        self.p = self.i = self.d = np.float32(0.0)

    def get_result(self, err):
        err = np.float32(err)
        self.i = np.float32(self.i + err)
        self.d = np.float32(err - self.p)
        self.p = err
        kp, ki, kd = self.k
        return np.float32(np.float32(np.float32(-kp * self.p) - np.float32(ki * self.i)) - np.float32(kd * self.d))


def _steering_control(ob_lib, lane, x, y, heading, hp, lp):
    """LaneChangePolicy.steering_control (lange_change_policy.py:62-71), with the lane geometry of the oracle"""
    lane = np.ascontiguousarray(np.asarray(lane).reshape(1))
    out = np.zeros(2, np.float32)
    ob_lib.ref_lane_local(lane.ctypes.data, x, y, out.ctypes.data)
    lng, lat = out
    lane_heading = ob_lib.ref_lane_heading_at(lane.ctypes.data, np.float32(lng + np.float32(1.0)))
    s = hp.get_result(-np.float32(ob_lib.ref_wrap_to_pi(np.float32(np.float32(lane_heading) - np.float32(heading)))))
    return np.float32(s + lp.get_result(-lat))


def _cxo_host():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    return HostScene(make_config(dict(lh.CXO_CONFIG, num_envs=1, build_workers=1)))


@pytest.mark.parametrize("lane_type", [0, 1])
def test_steering_matches_steering_control(lane_type):
    import oracle_binding as ob
    lib = ob.load()
    lanes = _cxo_host().world.arrays["lanes"]
    lane = lanes[np.nonzero(lanes["type"] == lane_type)[0][0]]
    rng = np.random.RandomState(lane_type)
    pid = np.zeros(1, abi.PID_DT)
    hp, lp = _Pid(1.7, 0.01, 3.5), _Pid(0.3, 0.002, 0.05)
    for t in range(40):       # points around the lane's start, a PID sequence of 40 steps
        x = np.float32(lane["sx"] + rng.uniform(-4, 4))
        y = np.float32(lane["sy"] + rng.uniform(-4, 4))
        h = np.float32(rng.uniform(-np.pi, np.pi))
        want = _steering_control(lib, lane, x, y, h, hp, lp)
        got = lh.steer(lane, x, y, h, pid)
        assert np.float32(got).tobytes() == want.tobytes(), (t, got, want)
        assert [pid[0][k] for k in ("hp", "hi", "hd", "lp", "li", "ld")] == [hp.p, hp.i, hp.d, lp.p, lp.i, lp.d]


def _synthetic_roads():
    """road 0: 2 lanes (ids 0, 1); road 1: 4 lanes (ids 2 .. 5)"""
    roads = np.zeros(2, abi.ROAD_DT)
    roads[0]["first_lane"], roads[0]["n_lanes"] = 0, 2
    roads[1]["first_lane"], roads[1]["n_lanes"] = 2, 4
    lanes = np.zeros(6, abi.LANE_DT)
    lanes["road"] = [0, 0, 1, 1, 1, 1]
    lanes["idx"] = [0, 1, 0, 1, 2, 3]
    lanes["n_in_road"] = [2, 2, 4, 4, 4, 4]
    return lanes, roads


def test_target_lanes():
    lanes, roads = _synthetic_roads()
    # on the reference road: left = index - 1 clamped at 0, right = index + 1 clamped at the last lane, keep = the lane
    assert [lh.target(lanes, roads, 0, 0, d) for d in (1, 0, -1)] == [0, 0, 1]
    assert [lh.target(lanes, roads, 1, 0, d) for d in (1, 0, -1)] == [0, 1, 1]
    # the current lane on another road: its index picks the reference road's lane
    assert [lh.target(lanes, roads, 3, 0, d) for d in (1, 0, -1)] == [0, 3, 1]


def test_target_lane_departures():
    lanes, roads = _synthetic_roads()
    # index - 1 past the reference road's lanes (the reference raises IndexError): its last lane
    assert lh.target(lanes, roads, 5, 0, 1) == 1
    assert lh.target(lanes, roads, 4, 0, 1) == 1
    # no current lane: no target; no reference road: the current lane
    assert [lh.target(lanes, roads, -1, 0, d) for d in (1, 0, -1)] == [-1, -1, -1]
    assert [lh.target(lanes, roads, 4, -1, d) for d in (1, 0, -1)] == [4, 4, 4]


def test_no_lane_is_not_steered():
    host = _cxo_host()
    lc = lh.LaneChangeOracle(host)
    lc.reset()
    lc.o.state["nav"]["lane"][0] = -1
    before = lc.pid.copy()
    applied = lc.step(np.array([[[1.0, 0.5]]], np.float32))
    assert applied[0, 0, 0] == 0.0 and applied[0, 0, 1] == np.float32(0.5)
    assert lc.pid.tobytes() == before.tobytes()


# ---- the reference's known answer on the oracle --------------------------------------------------------------------------
def _cxo_legs(legs):
    """test_lane_change (tests/test_policy/test_lane_change_policy.py:62-91): the env is stepped on through the whole run
    without a reset, whatever it reports (auto_reset=False: the reference's loop ignores `terminated` too)."""
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    from metadrive_ped_amd.envs.metadrive_env import discrete_to_continuous
    cfg = make_config(dict(lh.CXO_CONFIG, num_envs=1, build_workers=1, auto_reset=False))
    host = HostScene(cfg)
    lc = lh.LaneChangeOracle(host)
    lc.reset()
    got = []
    for act, n, _ in legs:
        decoded = discrete_to_continuous(torch, cfg, np.asarray(act), (1, ), "cpu").numpy().reshape(1, 1, 2)
        for _ in range(n):
            lc.step(decoded)
        got.append(lh.lane_index(host, lc.state))
    return got


def test_lane_change_known_answer_left_then_right():
    """59 steps of [2, 3] end on lane index 0, then 39 of [0, 3] on lane index 2."""
    assert _cxo_legs(lh.CXO_LEGS[:2]) == [0, 2]


@pytest.mark.xfail(strict=True, reason="the kinematic car reaches the X block 40 % faster than the reference's physics car: at step "
                   "158 it enters the block's curved entry lanes at the 80 km/h cap and cannot hold lane index 2 there with the "
                   "steering clipped to 1 (EXPERIMENTS.md, LaneChangePolicy)")
def test_lane_change_known_answer():
    """The whole reference answer: then 69 steps of [1, 3] stay on lane index 2."""
    assert _cxo_legs(lh.CXO_LEGS) == [0, 2, 2]


# ---- multi-agent --------------------------------------------------------------------------------------------------------
def test_roundabout_rollout_on_oracle():
    """Roundabout, 40 agents with respawns: every agent steered by its own PIDs; a respawned agent starts from clean ones."""
    from metadrive_ped_amd.engine import HostScene
    from metadrive_ped_amd.envs import BatchedMultiAgentRoundaboutEnv
    E, A = 2, 40
    cfg = BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, num_scenarios=E, agent_policy="LaneChangePolicy", discrete_action=True,
                                              build_workers=1)).config
    host = HostScene(cfg)
    lc = lh.LaneChangeOracle(host)
    lc.reset()
    rng = np.random.RandomState(5)
    rows = lc.agent_rows()
    steered = changed = 0
    idx0 = np.array([lh.lane_index(host, lc.state, e, a) for e in range(E) for a in range(A)])
    for t in range(150):
        d = np.zeros((E, A, 2), np.float32)
        d[..., 0] = rng.randint(-1, 2, (E, A))
        d[..., 1] = 0.5
        ids = lc.state["agent_id"][rows].copy()
        applied = lc.step(d)
        steered += int((~np.isin(applied[..., 0], [-1.0, 0.0, 1.0])).sum())
        fresh = lc.state["agent_id"][rows] != ids
        for k in lh.PID_ERRS:
            assert (lc.pid[k][rows][fresh] == 0.0).all()
        assert np.isfinite(lc.state["obs"]).all()
        if t == 60:
            idx = np.array([lh.lane_index(host, lc.state, e, a) for e in range(E) for a in range(A)])
            changed = int((idx != idx0).sum())
    assert steered > 1000 and changed > 0
    assert (lc.state["next_agent_id"] > A).all()            # respawns happened
