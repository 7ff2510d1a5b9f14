"""agent_policy = LaneChangePolicy on the device: bit-exact parity of the step kernels (workgroup RESPAWN variant,
wave_step_kernel<true>, the MULTI variant) with the CPU oracle driven by the host restatement of include/md_lane_change.h
(tests/lane_change_host.py).  The agents' PID rows are compared with the restatement's, everything else with the oracle's."""
import numpy as np
import pytest

import lane_change_host as lh
from helpers import assert_state_equal
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

SINGLE_KEYS = ["shape", "dyn", "nav", "pid", "action", "flags", "obs", "reward", "cost", "step_info", "need_reset", "route_nodes",
               "route_roads", "final_lane"]
MULTI_KEYS = SINGLE_KEYS + ["rng", "env_steps", "agent_id", "next_agent_id"]


def _expected(lc):
    """the oracle's state with the restatement's PID errors in the agents' rows"""
    ref = {k: v.copy() for k, v in lc.state.items()}
    rows = lc.agent_rows()
    for k in lh.PID_ERRS:
        ref["pid"][k][rows] = lc.pid[k][rows]
    return ref


def _directions(rng, E, A):
    d = np.zeros((E, A, 2), np.float32)
    d[..., 0] = rng.randint(-1, 2, (E, A))
    d[..., 1] = rng.choice(np.float32([-0.5, 0.0, 0.5, 1.0]), (E, A))
    return d


def _run(eng, lc, steps, keys, seed, check_every=25):
    import torch
    E, A = eng.host.E, eng.host.A
    rng = np.random.RandomState(seed)
    resets = 0
    for t in range(steps):
        d = _directions(rng, E, A)
        resets += int(lc.state["need_reset"].sum())
        eng.step(torch.from_numpy(d).to(eng.device))
        lc.step(d)
        if t % check_every == 0 or t == steps - 1:
            assert_state_equal(eng.download_state(), _expected(lc), keys=keys, where="step %d" % t)
    return resets


@pytest.mark.parametrize("kernel", ["wg", "wave"])
def test_single_agent_parity(kernel):
    """traffic on, auto-resets (a short horizon), both single-agent step kernels"""
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    E = 24
    cfg = make_config(dict(num_envs=E, num_scenarios=E, start_seed=100, traffic_density=0.2, horizon=60, agent_policy="LaneChangePolicy",
                           discrete_action=True, step_kernel=kernel))
    eng = BatchedEngine(cfg)
    assert eng.k.agent_idm == abi.AGENT_LANE_CHANGE
    lc = lh.LaneChangeOracle(eng.host)
    eng.reset()
    lc.reset()
    assert_state_equal(eng.download_state(), _expected(lc), keys=SINGLE_KEYS, where="reset")
    resets = _run(eng, lc, 200, SINGLE_KEYS, seed=1)
    assert resets >= E                                           # every env went through at least one auto-reset
    rows = lc.agent_rows()
    assert np.abs(eng.download_state()["pid"]["lp"][rows]).max() > 0.0


def test_multi_agent_parity():
    """roundabout, 40 agents, respawns: the MULTI variant"""
    from metadrive_ped_amd.engine import BatchedEngine
    from metadrive_ped_amd.envs import BatchedMultiAgentRoundaboutEnv
    E = 6
    cfg = BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, num_scenarios=E, agent_policy="LaneChangePolicy", discrete_action=True,
                                              vehicle_config=dict(lidar=dict(num_lasers=240, distance=50)))).config
    eng = BatchedEngine(cfg)
    lc = lh.LaneChangeOracle(eng.host)
    eng.reset()
    lc.reset()
    _run(eng, lc, 200, MULTI_KEYS, seed=2)
    assert (lc.state["next_agent_id"] > eng.host.A).all()       # respawns happened


def test_state_checkpoint_keeps_the_pids():
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    E = 8
    env = BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=E, traffic_density=0.1, agent_policy="LaneChangePolicy",
                                   discrete_action=True, use_multi_discrete=True))
    env.reset()
    rng = np.random.RandomState(4)
    acts = [rng.randint(0, [3, 5], (E, 2)) for _ in range(60)]
    for a in acts[:30]:
        env.step(torch.from_numpy(a))
    st = env.get_state()
    assert np.abs(st["pid"]["hp"].reshape(E, -1)[:, 0]).max() > 0.0
    first = []
    for a in acts[30:]:
        obs = env.step(torch.from_numpy(a))[0]
        first.append(obs.cpu().numpy().copy())
    end = env.get_state()
    env.set_state(st)
    for a, want in zip(acts[30:], first):
        obs = env.step(torch.from_numpy(a))[0]
        assert obs.cpu().numpy().tobytes() == want.tobytes()
    again = env.get_state()
    for k in ("pid", "shape", "dyn", "nav"):
        assert again[k].tobytes() == end[k].tobytes(), k


def test_cxo_known_answer_through_env():
    """The reference's test_lane_change through BatchedMetaDriveEnv: the first two legs' lanes, and the device trajectory
    equal to the oracle + restatement's to the end of the third leg (see tests/test_lane_change.py for that leg's lane)."""
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    from metadrive_ped_amd.envs.metadrive_env import discrete_to_continuous
    env = BatchedMetaDriveEnv(dict(lh.CXO_CONFIG, num_envs=1, auto_reset=False))
    env.reset()
    lc = lh.LaneChangeOracle(env.engine.host)
    lc.reset()
    lanes = []
    for act, n, _ in lh.CXO_LEGS:
        for _ in range(n):
            env.step(np.asarray(act))
            lc.step(discrete_to_continuous(torch, env.config, np.asarray(act), (1, ), "cpu").numpy().reshape(1, 1, 2))
        st = env.engine.download_state()
        assert_state_equal(st, _expected(lc), keys=SINGLE_KEYS, where="after %s" % act)
        lanes.append(lh.lane_index(env.engine.host, st))
    assert lanes[:2] == [0, 2]


def test_md_step_refuses_unknown_policy():
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    eng = BatchedEngine(make_config(dict(num_envs=2, num_scenarios=2, agent_policy="LaneChangePolicy", discrete_action=True)))
    eng.reset()
    eng.k.agent_idm = 3
    with pytest.raises(Exception, match="agent_idm=3"):
        eng.step(torch.zeros((2, 1, 2), device=eng.device))
