"""config["expert_own_sensors"] (the expert observes through its own sensors, md_expert_sense): what the key accepts, what stays
refused by name, the entry point's table, and the observation layout the refactored md_observe_combine writes (the oracle's golden
and parity suites pin the bits; here the layout function it now shares is checked through the oracle on a small batch)."""
import numpy as np
import pytest

import expert_host as eh

OTHER_SENSORS = dict(random_agent_model=True, vehicle_config=dict(lidar=dict(num_lasers=72, distance=40, num_others=2),
                                                                  side_detector=dict(num_lasers=12)))


def test_key_accepts_any_vehicle_config():
    from metadrive_ped_amd.config import make_config
    cfg = make_config(dict(OTHER_SENSORS, agent_policy="ExpertPolicy", expert_own_sensors=True))
    assert cfg["expert_own_sensors"] is True and cfg["agent_policy"] == "ExpertPolicy"
    assert make_config({})["expert_own_sensors"] is False


def test_without_the_key_the_old_refusal_stands():
    from metadrive_ped_amd.config import make_config
    with pytest.raises(ValueError, match="num_lasers") as ei:
        make_config(dict(OTHER_SENSORS, agent_policy="ExpertPolicy"))
    assert "numpy_expert.py" in str(ei.value) and "expert_own_sensors=True" in str(ei.value)
    with pytest.raises(ValueError, match="num_lasers"):
        make_config(dict(OTHER_SENSORS, agent_policy="ExpertPolicy", expert_own_sensors=False))


def test_refusals_by_name():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentTollgateEnv
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    with pytest.raises((ValueError, NotImplementedError), match="ExpertPolicy.*BatchedScenarioEnv"):
        BatchedScenarioEnv(dict(agent_policy="ExpertPolicy", expert_own_sensors=True))
    with pytest.raises(ValueError, match="ExpertPolicy.*tollgate"):
        BatchedMultiAgentTollgateEnv(dict(agent_policy="ExpertPolicy", expert_own_sensors=True))
    with pytest.raises(NotImplementedError, match="AIProtectPolicy.*expert_own_sensors"):
        make_config(dict(agent_policy="AIProtectPolicy", expert_own_sensors=True))
    with pytest.raises(NotImplementedError, match="AIProtectPolicy.*expert_own_sensors"):
        make_config(dict(OTHER_SENSORS, agent_policy="AIProtectPolicy", expert_own_sensors=True))


def test_expert_function_takes_the_key_per_call():
    from metadrive_ped_amd.config import expert_config_problem, make_config
    from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentRoundaboutEnv, BatchedMultiAgentTollgateEnv
    cfg = make_config(OTHER_SENSORS)
    assert "num_lasers" in expert_config_problem(cfg)
    assert expert_config_problem(cfg, own_sensors=True) is None
    assert "num_lasers" in expert_config_problem(make_config(dict(OTHER_SENSORS, expert_own_sensors=True)), own_sensors=False)
    assert expert_config_problem(BatchedMultiAgentRoundaboutEnv().config, own_sensors=True) is None
    assert "tollgate" in expert_config_problem(BatchedMultiAgentTollgateEnv().config, own_sensors=True)


def test_multi_agent_classes_accepted():
    from metadrive_ped_amd.envs import marl_env as m
    for cls in (m.BatchedMultiAgentRoundaboutEnv, m.BatchedMultiAgentIntersectionEnv, m.BatchedMultiAgentTinyInter,
                m.BatchedMultiAgentRacingEnv, m.BatchedMultiAgentBottleneckEnv, m.BatchedMultiAgentBidirectionEnv,
                m.BatchedMultiAgentParkingLotEnv, m.BatchedMultiAgentMetaDrive):
        env = cls(dict(agent_policy="ExpertPolicy", expert_own_sensors=True, expert_weights=eh.WEIGHTS))
        assert env.config["agent_policy"] == "ExpertPolicy" and env.config["is_multi_agent"]
        with pytest.raises((ValueError, NotImplementedError), match="ExpertPolicy.*multi-agent"):
            cls(dict(agent_policy="ExpertPolicy"))


def test_entry_point_has_a_table_of_its_own():
    from metadrive_ped_amd import abi
    assert list(abi.EXPERT_SENSE_ENTRY_POINTS) == ["md_expert_sense"]
    for table in (abi.ENTRY_POINTS, abi.EXPERT_ENTRY_POINTS, abi.AI_PROTECT_ENTRY_POINTS, abi.CURRICULUM_ENTRY_POINTS):
        assert "md_expert_sense" not in table
    assert len(abi.EXPERT_SENSE_ENTRY_POINTS["md_expert_sense"][1]) == 10
    assert abi.MD_ABI_VERSION == 12


def test_only_an_own_sensors_policy_batch_goes_without_detected_sets():
    """the obs-row expert needs MdState.detected (and with it md_step's general variant); the own-sensors expert keeps its sets in
    LDS, so its batch steps with the lean kernel"""
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    base = dict(num_envs=2, map="S", traffic_density=0.0, build_workers=1, agent_policy="ExpertPolicy")
    assert "detected" in HostScene(make_config(base)).state
    assert "detected" not in HostScene(make_config(dict(base, expert_own_sensors=True))).state


def test_oracle_rows_under_every_layout_keep_their_blocks():
    """md_observe_combine now writes the dims before the "others" block through md_observe_state_dims: under the layouts that move
    those dims (random_agent_model's two size dims, detectors that own dims) the oracle's rows are finite, the size dims are the
    vehicle's, and the state dims of the plain layout equal the same dims of the shifted one bit for bit."""
    import oracle_binding as ob
    from helpers import scripted_actions
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    base = dict(num_envs=3, num_scenarios=3, map="SC", traffic_density=0.1, build_workers=1, start_seed=4)
    plain = ob.OracleWorld(HostScene(make_config(base)))
    # the same scenes observed with two more detectors: the vehicles and the traffic are the same (the detectors draw nothing)
    det = ob.OracleWorld(HostScene(make_config(dict(base, vehicle_config=dict(side_detector=dict(num_lasers=4),
                                                                             lane_line_detector=dict(num_lasers=2))))))
    plain.reset()
    det.reset()
    for t in range(12):
        a = scripted_actions(3, 1, t, seed=2)
        plain.step(a)
        det.step(a)
        p, d = plain.obs, det.obs
        assert p.shape == (3, 259) and d.shape == (3, 259 + 2 + 1) and np.isfinite(p).all() and np.isfinite(d).all()
        # heading .. yaw rate: [2, 8) plain, [4, 10) behind a 4-beam side detector; navi [9, 19) plain, [12, 22) behind both
        assert np.array_equal(p[:, 2:8].view(np.uint32), d[:, 4:10].view(np.uint32)), t
        assert np.array_equal(p[:, 9:19].view(np.uint32), d[:, 12:22].view(np.uint32)), t
        assert np.array_equal(p[:, 19:].view(np.uint32), d[:, 22:].view(np.uint32)), t
