"""agent_policy="AIProtectPolicy" (include/md_ai_protect.h) without a GPU: the host build of the rule against the reference's own
AIProtectPolicy.act (tests/golden/ai_protect.npz, tools/gen_ai_protect_golden.py), the config rules, and a rollout on the CPU oracle
with the host expert as the saver."""
import numpy as np
import pytest

import ai_protect_host as ah
import expert_host as eh

NEAR = 1e-5       # the golden's near-tie margin: float64 comparisons of the reference against float32 ones here


@pytest.fixture(scope="module")
def golden():
    with np.load(ah.GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host_inputs(g):
    """MdProtectIn of every golden case from its stored inputs: heading_diff by the header on the case's MdLane record, the window
    minima by the header on the case's cloud."""
    n = len(g["save_level"])
    ins = np.zeros(n, ah.IN_DT)
    for i in range(n):
        kind = "straight" if g["lane_type"][i] == 0 else "circular"
        L = ah.lane_record(kind, **{k: g["lane_" + k][i] for k in ("sx", "sy", "ex", "ey", "ax", "ay", "dirsign")})
        ins["heading_diff"][i] = ah.heading_diff(L, 0, *g["pos"][i], *g["heading"][i])
        ins["lat_min"][i], ins["lon_min"][i] = ah.windows(g["cloud"][i])
    ins["obs0"], ins["obs1"] = g["obs012"][:, 0], g["obs012"][:, 1]
    ins["speed_kmh"], ins["max_speed_kmh"] = g["speed_km_h"], g["max_speed_km_h"]
    return ins


def _flags(g):
    return (g["info_takeover"] * ah.TAKEOVER + g["info_start"] * ah.TAKEOVER_START + g["info_end"] * ah.TAKEOVER_END).astype(np.uint8)


def test_golden_covers_what_it_should(golden):
    g = golden
    n = len(g["save_level"])
    assert 500 <= n <= 700
    assert set(np.round(g["save_level"], 6)) == {0.0, 1e-3, 0.05, 0.3, 0.5, 0.9, 0.95, 1.0}
    assert (g["margin"] <= NEAR).sum() <= 0.02 * n
    assert g["expert_takeover"].sum() >= 30
    assert (g["speed_km_h"] < 5).any() and (g["speed_km_h"] >= 5).any()
    fl = _flags(g)
    assert {0, ah.TAKEOVER, ah.TAKEOVER_START, ah.TAKEOVER_END} <= set(fl.tolist())
    for c in range(int(g["chain"].max()) + 1):      # a chain is one vehicle: each call starts from the state the last one left
        m = np.nonzero(g["chain"] == c)[0]
        assert np.array_equal(g["pre_takeover"][m][1:], g["takeover_after"][m][:-1])
    assert (g["lane_type"] == 0).any() and (g["lane_dirsign"] > 0).any() and (g["lane_dirsign"] < 0).any()


def test_heading_diff_is_the_references_on_vehicle_lane(golden):
    """BaseVehicle.heading_diff on real lanes of both kinds and senses within float32 rounding; it is taken on vehicle.lane, which
    in the golden differs from the lane observation dim 2 looks at."""
    ins = _host_inputs(golden)
    assert np.abs(ins["heading_diff"] - golden["heading_diff"]).max() < 2e-6
    assert (np.abs(golden["obs012"][:, 2] - golden["heading_diff"]) > 0.05).sum() > 100


def test_rule_matches_reference_golden(golden):
    g = golden
    keep = g["margin"] > NEAR
    assert (~keep).sum() <= 0.02 * len(keep)
    ins = _host_inputs(g)
    applied, flags, after = ah.act(g["action"], g["saver_a"], ins, g["save_level"], g["expert_takeover"], g["pre_takeover"])
    assert np.array_equal(flags[keep], _flags(g)[keep])
    assert np.array_equal(after[keep].astype(bool), g["takeover_after"][keep])
    bad = np.nonzero((_f32_bits(applied) != _f32_bits(g["out_action"])).any(1) & keep)[0]
    assert bad.size == 0, bad
    # what would differ had the rule looked at the observation's lane instead of vehicle.lane
    other = ins.copy()
    other["heading_diff"] = g["obs012"][:, 2]
    _, fl2, _ = ah.act(g["action"], g["saver_a"], other, g["save_level"], g["expert_takeover"], g["pre_takeover"])
    assert (fl2 != flags).any()


def test_windows_are_half_open():
    """min(lidar_p[left - 4:left + 6]), [right - 4:right + 6], [0:10], [-10:] with left = 60, right = 180"""
    for idx, lat, lon in ((55, 1, 1), (56, 0, 1), (65, 0, 1), (66, 1, 1), (175, 1, 1), (176, 0, 1), (185, 0, 1), (186, 1, 1),
                          (0, 1, 0), (9, 1, 0), (10, 1, 1), (229, 1, 1), (230, 1, 0), (239, 1, 0)):
        c = np.ones(240, np.float32)
        c[idx] = 0.25
        got = ah.windows(c)
        assert got == (np.float32(0.25) if not lat else 1.0, np.float32(0.25) if not lon else 1.0), idx


def test_reset_env_passes_the_action_and_clears_both_bytes():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(make_config(dict(num_envs=2, map="C", traffic_density=0.0, agent_policy="AIProtectPolicy", save_level=1.0,
                                      build_workers=1)))
    st = host.clone_state()
    assert st["takeover"].dtype == np.uint8 and st["takeover"].shape == (2, ) and st["expert_takeover"].shape == (2, )
    st["need_reset"][:] = (1, 0)
    tk, et = np.ones(2, np.uint8), np.array([1, 0], np.uint8)
    raw = np.float32([[3.0, -2.0], [3.0, -2.0]])
    sv = np.float32([[0.1, 0.2], [0.1, 0.2]])
    applied, flags, _ = ah.batch(host.world.arrays, st, host.md_config, st["obs"], raw, sv, 1.0, tk, et)
    assert applied[0].tolist() == [3.0, -2.0] and flags[0] == 0 and tk[0] == 0 and et[0] == 0
    assert applied[1].tolist() == [np.float32(0.1), np.float32(0.2)] and flags[1] == ah.TAKEOVER and tk[1] == 1


# -- config ------------------------------------------------------------------------------------------------------------
def test_ai_protect_policy_accepted():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv, BatchedSafeMetaDriveEnv, BatchedVaryingDynamicsEnv
    for cls in (BatchedMetaDriveEnv, BatchedSafeMetaDriveEnv, BatchedVaryingDynamicsEnv):
        env = cls(dict(agent_policy="AIProtectPolicy", expert_weights=eh.WEIGHTS))
        assert env.config["agent_policy"] == "AIProtectPolicy" and env.config["save_level"] == 0.5
        assert env.observation_space.shape == (259, ) and env.action_space.shape == (2, )

    class AIProtectPolicy:     # the reference passes the class
        pass

    assert make_config(dict(agent_policy=AIProtectPolicy))["agent_policy"] == "AIProtectPolicy"
    for level in (0.0, 1e-3, 0.3, 1, 1.0):
        assert make_config(dict(agent_policy="AIProtectPolicy", save_level=level))["save_level"] == level


def test_save_level_rules():
    from metadrive_ped_amd.config import make_config
    assert make_config(dict(save_level=0.5))["save_level"] == 0.5
    with pytest.raises(NotImplementedError, match="save_level.*AIProtectPolicy"):
        make_config(dict(save_level=0.3))
    with pytest.raises(NotImplementedError, match="save_level"):
        make_config(dict(save_level=0.3, agent_policy="ExpertPolicy"))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="save_level"):
            make_config(dict(agent_policy="AIProtectPolicy", save_level=bad))
    with pytest.raises(NotImplementedError, match="use_AI_protector.*agent_policy='AIProtectPolicy'"):
        make_config(dict(use_AI_protector=True))
    with pytest.raises(NotImplementedError, match="use_AI_protector"):
        make_config(dict(use_AI_protector=True, agent_policy="AIProtectPolicy"))


def test_ai_protect_policy_needs_the_experts_observation():
    from metadrive_ped_amd.config import make_config
    with pytest.raises(ValueError, match="num_lasers") as ei:
        make_config(dict(agent_policy="AIProtectPolicy", vehicle_config=dict(lidar=dict(num_lasers=120))))
    assert "numpy_expert.py" in str(ei.value)
    with pytest.raises(ValueError, match="random_agent_model"):
        make_config(dict(agent_policy="AIProtectPolicy", random_agent_model=True))


def test_ai_protect_policy_refused_in_other_envs():
    from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentMetaDrive, BatchedMultiAgentRoundaboutEnv
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    with pytest.raises((ValueError, NotImplementedError), match="AIProtectPolicy.*multi-agent"):
        BatchedMultiAgentRoundaboutEnv(dict(agent_policy="AIProtectPolicy"))
    with pytest.raises((ValueError, NotImplementedError), match="AIProtectPolicy.*multi-agent"):
        BatchedMultiAgentMetaDrive(dict(agent_policy="AIProtectPolicy"))
    with pytest.raises((ValueError, NotImplementedError), match="AIProtectPolicy.*BatchedScenarioEnv"):
        BatchedScenarioEnv(dict(agent_policy="AIProtectPolicy"))


def test_expert_takeover_belongs_to_the_policy():
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict())
    with pytest.raises(ValueError, match="AIProtectPolicy"):
        env.set_expert_takeover(True)
    env = BatchedMetaDriveEnv(dict(agent_policy="AIProtectPolicy"))
    with pytest.raises(RuntimeError, match="reset"):
        env.set_expert_takeover(True)


# -- a rollout on the CPU oracle: the host expert + the host rule guard an agent that steers off the road --------------------
def _rollout(weights, save_level, steps):
    """-> (flag bytes per step, the step at which the episode ended out of road or None)"""
    import oracle_binding as ob
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    # the expert's own observation config for the oracle (num_others = 4): its obs row is the expert's raw observation
    host = HostScene(make_config(dict(num_envs=1, map="S", traffic_density=0.0, num_scenarios=1, start_seed=2, build_workers=1,
                                      random_spawn_lane_index=False, vehicle_config=dict(lidar=dict(num_others=4)))))
    o = ob.OracleWorld(host)
    o.reset()
    tk, et = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    noise = np.random.RandomState(3).standard_normal((steps, 1, 2)).astype(np.float32)
    k259 = host.md_config.__class__.from_buffer_copy(host.md_config)
    k259.obs_dim = 259
    flags = []
    for t in range(steps):
        raw275 = o.obs[0].copy()
        _, out = eh.expert(weights, raw275)
        sv = eh.sample(out, noise[t])
        row = np.concatenate([raw275[:19], raw275[35:]])[None]          # the env's own observation: state | cloud
        st = dict(o.state, need_reset=np.zeros(1, np.int32))
        applied, fl, _ = ah.batch(host.world.arrays, st, k259, row, np.float32([[0.6, 0.8]]), sv, save_level, tk, et)
        flags.append(int(fl[0]))
        o.step(applied.reshape(1, 1, 2))
        word = int(o.state["flags"][0])
        if word & (abi.FL_TERMINATED | abi.FL_TRUNCATED):
            return flags, (t if word & abi.FL_OUT_OF_ROAD else None)
    return flags, None


def test_saver_keeps_the_agent_on_the_road():
    """An agent that steers left at 0.6 with throttle 0.8 on a straight road: unguarded (save_level 0) it ends out of road; guarded
    at save_level 0.5 the takeover flags obey start -> hold -> end and the episode does not end out of road within those steps."""
    weights = eh.packed_weights()
    flags0, out0 = _rollout(weights, 0.0, 400)
    assert out0 is not None and not any(flags0), (out0, flags0)
    flags, out = _rollout(weights, 0.5, out0 + 1)
    assert out is None, out
    assert any(f == ah.TAKEOVER_START for f in flags) and any(f == ah.TAKEOVER for f in flags)
    state = 0          # 0 = free, 1 = started / holding
    for f in flags:
        assert f in (0, ah.TAKEOVER, ah.TAKEOVER_START, ah.TAKEOVER_END), f      # one bit at a time
        if state == 0:
            assert f in (0, ah.TAKEOVER_START), flags
        else:
            assert f in (ah.TAKEOVER, ah.TAKEOVER_END), flags
        state = 1 if f in (ah.TAKEOVER_START, ah.TAKEOVER) else 0
