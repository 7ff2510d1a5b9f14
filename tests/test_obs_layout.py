"""ObsLayout is the one place the host layer computes where the dims of an observation row sit (the mirror of md_obs_* in
include/md_entity.h and md_sc_obs_* in include/md_scenario.h).  For a matrix of configs: the env's observation_space, the layout
and the host scene agree on obs_dim; the offsets are ordered and fill the row; and obs_dim has the value worked out by hand from
the reference's obs/state_obs.py:64-151 and marl_tollgate.py:62-110 (the same values the env classes gave before the layout was
single-sourced)."""
import pytest

from metadrive_ped_amd import envs as E
from metadrive_ped_amd.engine import HostScene
from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
from metadrive_ped_amd.obs_layout import ObsLayout
from metadrive_ped_amd.scenario import ScenarioHostScene


def _vc(**kw):
    return dict(vehicle_config=kw)


LIDAR_OFF = dict(lidar=dict(distance=0))
SIDE, LANE_LINE = dict(side_detector=dict(num_lasers=12, distance=50)), dict(lane_line_detector=dict(num_lasers=4, distance=20))

# (env class, user config, pinned obs_dim or None)
SINGLE = [
    ("default", {}, 259),
    ("lidar_off", _vc(**LIDAR_OFF), 19),
    ("random_agent_model", dict(random_agent_model=True), 261),
    ("others4", _vc(lidar=dict(num_others=4)), 275),                 # the expert's observation width, MD_EXPERT_IN
    ("others4_navi", _vc(lidar=dict(num_others=4, add_others_navi=True)), 291),
    ("others4_lidar_off", _vc(lidar=dict(num_others=4, add_others_navi=True, distance=0)), 19),    # no lidar, no others block
    ("side", _vc(**SIDE), 259 - 2 + 12),
    ("lane_line", _vc(**LANE_LINE), 259 - 1 + 4),
    ("side_lane_line", _vc(**SIDE, **LANE_LINE), 259 - 3 + 16),
    ("side_lane_line_lidar_off", _vc(**SIDE, **LANE_LINE, **LIDAR_OFF), 19 - 3 + 16),
    ("detectors_distance_0", _vc(side_detector=dict(num_lasers=12, distance=0), lane_line_detector=dict(num_lasers=4, distance=0)), 259),
    ("everything", dict(random_agent_model=True, **_vc(lidar=dict(num_others=4, add_others_navi=True), **SIDE, **LANE_LINE)), 2 + 12 + 6 + 4 + 10 + 32 + 240),
]
MARL = [
    (E.BatchedMultiAgentRoundaboutEnv, 91), (E.BatchedMultiAgentIntersectionEnv, 91), (E.BatchedMultiAgentParkingLotEnv, 91),
    (E.BatchedMultiAgentTinyInter, 91), (E.BatchedMultiAgentMetaDrive, 91), (E.BatchedMultiAgentBottleneckEnv, 96),
    (E.BatchedMultiAgentBidirectionEnv, 96), (E.BatchedMultiAgentTollgateEnv, 156), (E.BatchedMultiAgentRacingEnv, 161),
]
SCENARIO = [("default", {}, 161), ("lidar_off", _vc(**LIDAR_OFF), 161 - 120), ("lane_line", _vc(**LANE_LINE), 161 - 1 + 4),
            ("side_off", _vc(side_detector=dict(distance=0)), 161 - 12 + 2)]


def _check(env, host, scenario, pinned):
    L = ObsLayout(env.config, scenario=scenario)
    assert env.observation_space.shape == (L.obs_dim, )
    assert host.obs_dim == L.obs_dim == host.layout.obs_dim and host.md_config.obs_dim == L.obs_dim
    for k in ObsLayout.HOST_ATTRS:
        assert getattr(host, k) == getattr(L, k), k
    # ordered and contiguous: base | side | 6 | lane-line | navi | others | lidar | tail
    assert L.side_off == L.obs_base and L.side_off <= L.mid_off < L.ll_off < L.navi_off <= L.others_off <= L.lidar_off
    assert L.mid_off - L.side_off == (L.n_side or 2) and L.ll_off - L.mid_off == 6 and L.navi_off - L.ll_off == (L.n_ll or 1)
    assert L.others_off - L.navi_off == L.navi_dims and L.others_off == L.state_dim
    assert L.lidar_off - L.others_off == L.others_dim == L.num_others * (8 if L.add_others_navi else 4)
    assert L.lidar_off + L.n_beams + L.tail == L.obs_dim
    assert L.obs_dim == pinned
    return L


@pytest.mark.parametrize("name,user,pinned", SINGLE, ids=[c[0] for c in SINGLE])
def test_single_agent_layout(name, user, pinned):
    env = E.BatchedMetaDriveEnv(dict(user, num_envs=2))
    L = _check(env, HostScene(env.config), False, pinned)
    assert L.navi_dims == 10 and L.tail == 0 and L.obs_base == (2 if env.config["random_agent_model"] else 0)
    if L.n_beams == 0:
        assert L.num_others == 0 and not L.add_others_navi


@pytest.mark.parametrize("cls,pinned", MARL, ids=[c[0].__name__ for c in MARL])
def test_marl_layout(cls, pinned):
    env = cls(dict(num_envs=1))
    assert env.observation_space.shape == (pinned, )
    if cls is E.BatchedMultiAgentRacingEnv:
        # the default 12 agents need exit_length >= 60 to find their spawn slots, as in the reference (its own tests pass 60):
        # the map's size is no part of the layout
        env = cls(dict(num_envs=1, map_config=dict(exit_length=60)))
    L = _check(env, HostScene(env.config), False, pinned)
    toll = cls is E.BatchedMultiAgentTollgateEnv
    assert (L.navi_dims, L.tail, L.tollgate) == ((0, 2, True) if toll else (10, 0, False))


def test_marl_random_agent_model_leads_with_two_dims():
    env = E.BatchedMultiAgentRoundaboutEnv(dict(num_envs=1, random_agent_model=True))
    assert _check(env, HostScene(env.config), False, 93).obs_base == 2


@pytest.mark.parametrize("name,user,pinned", SCENARIO, ids=[c[0] for c in SCENARIO])
def test_scenario_layout(name, user, pinned):
    env = BatchedScenarioEnv(dict(user, num_envs=2))          # synthetic scenes
    L = _check(env, ScenarioHostScene(env.config, env.scenarios), True, pinned)
    assert L.navi_dims == 22 and L.obs_base == 0 and L.num_others == 0 and L.tail == 0
    assert ObsLayout(env.config).obs_dim == L.obs_dim         # scenario=None reads config["scenario_mode"]


def test_scenario_mode_ignores_agent_model_and_others():
    env = BatchedScenarioEnv(dict(num_envs=2))
    cfg = dict(env.config, random_agent_model=True)
    cfg["vehicle_config"] = dict(cfg["vehicle_config"], lidar=dict(cfg["vehicle_config"]["lidar"], num_others=4))
    L = ObsLayout(cfg, scenario=True)
    assert (L.obs_base, L.num_others, L.obs_dim) == (0, 0, 161)
