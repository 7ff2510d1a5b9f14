"""The scenario walk on the device: md_step + md_swap_draw (scenario_step_kernel reading the per-scene tables through
MdState.scene_of, swap_draw_kernel moving envs on) bit for bit against the oracle stepped with the same swap (tests/walk_host.py),
over several episode ends per env; info["scenario_index"]; reproducible uniform draws; checkpoints taken mid-walk."""
import numpy as np
import pytest

import walk_host as wh
from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config, synthetic_scenarios

pytestmark = pytest.mark.gpu

T_FRAMES = 80
KEYS = ["shape", "dyn", "nav", "pid", "param", "action", "flags", "obs", "reward", "cost", "step_info", "need_reset", "next_agent_id",
        "shape0", "dyn0", "scene_of", "walk_ep"]
ROUTE_KEYS = ["route_n", "route_segs", "route_verts", "route_aux"]


def _follow(obs, n_side=12):
    o_navi = (n_side or 2) + 6 + 1
    a = np.zeros((len(obs), 1, 2), np.float32)
    a[:, 0, 0] = np.clip(6.0 * (obs[:, o_navi + 19] - 0.5) + 2.0 * (obs[:, o_navi + 18] - 0.5), -1, 1)
    a[:, 0, 1] = 0.3
    return a


_POOLS = {}


def _pool(n):
    if n not in _POOLS:
        _POOLS[n] = synthetic_scenarios(n, 900, T=T_FRAMES)
    return _POOLS[n]


@pytest.mark.parametrize("seq,reactive,E,n", [(True, True, 4, 9), (False, False, 4, 3), (True, False, 1024, 300),
                                               (False, True, 1024, 300), (True, True, 4, 2)])
def test_walk_gpu_parity(seq, reactive, E, n):
    import torch
    from helpers import assert_state_equal
    from metadrive_ped_amd.engine import BatchedEngine
    horizon = 18
    cfg = make_scenario_config(dict(num_envs=E, num_scenarios=n, walk_scenarios=True, sequential_seed=seq, horizon=horizon,
                                    reactive_traffic=reactive, start_seed=11))
    host = ScenarioHostScene(cfg, _pool(n))
    eng = BatchedEngine(cfg, host=host)
    o = wh.WalkOracle(host)
    eng.reset()
    o.reset()
    keys = KEYS + (ROUTE_KEYS if reactive else [])
    assert_state_equal(eng.download_state(), o.state, keys=keys, where="walk reset")
    rng = np.random.RandomState(5)
    for t in range(4 * (horizon + 1) + 2):
        a = _follow(o.obs)
        a[:, 0, 0] += rng.uniform(-0.1, 0.1, size=E).astype(np.float32)
        eng.step(torch.from_numpy(a).to(eng.device))
        o.step(a)
        if t % 10 == 0 or t > 4 * horizon:
            assert_state_equal(eng.download_state(), o.state, keys=keys, where="walk step %d" % t)
            env_map = eng.world_dev["env_map"].view(torch.int32).cpu().numpy()
            assert np.array_equal(env_map, o.env_map), t
    st = eng.download_state()
    assert (st["walk_ep"] >= 3).all()
    assert np.array_equal(st["scene_of"], wh.cfg_walk_scene(cfg, np.arange(E), st["walk_ep"]))


def test_info_scenario_index_follows_the_schedule_and_draws_repeat():
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    E, n, start = 8, 13, 40
    runs = []
    for _ in range(2):
        env = BatchedScenarioEnv(dict(num_envs=E, num_scenarios=n, start_scenario_index=start, walk_scenarios=True, horizon=8,
                                      sequential_seed=False, start_seed=2), scenarios=_pool(n))
        obs, info = env.reset()
        ep = np.zeros(E, np.int64)
        seen = [info["scenario_index"].cpu().numpy()]
        assert np.array_equal(seen[0], start + wh.cfg_walk_scene(env.config, np.arange(E), 0))
        for t in range(60):
            obs, r, term, trunc, info = env.step(torch.from_numpy(_follow(obs.cpu().numpy())[:, 0]).to(env.engine.device))
            idx = info["scenario_index"].cpu().numpy()
            assert np.array_equal(idx, start + wh.cfg_walk_scene(env.config, np.arange(E), ep)), t
            seen.append(idx)
            ep += (term | trunc).cpu().numpy().astype(np.int64)
        runs.append(np.stack(seen))
        env.close()
    assert np.array_equal(runs[0], runs[1])          # reproducible
    assert set(np.unique(runs[0]).tolist()) == set(range(start, start + n))   # over the whole slice


def test_walk_checkpoint_resumes_exactly_and_refuses_another_slice():
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    E, n = 6, 10

    def make(start=0):
        return BatchedScenarioEnv(dict(num_envs=E, num_scenarios=n, start_scenario_index=start, walk_scenarios=True, horizon=10,
                                       reactive_traffic=True, sequential_seed=True), scenarios=_pool(n))

    def act(obs):
        return torch.from_numpy(_follow(obs.cpu().numpy())[:, 0]).to(env.engine.device)
    env = make()
    obs, _ = env.reset()
    for _ in range(27):
        obs = env.step(act(obs))[0]
    st = env.get_state()
    assert (st["walk_ep"] >= 2).all()
    outs = []
    for _ in range(30):
        o, r, te, tr, info = env.step(act(obs))
        outs.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), info["scenario_index"].cpu().numpy()))
        obs = o
    env2 = make()
    env2.reset()
    for _ in range(5):
        env2.step(act(env2.engine.obs[:, 0, :]))
    env2.set_state(st)
    obs = env2.engine.obs[:, 0, :]
    for t in range(30):
        o, r, te, tr, info = env2.step(act(obs))
        assert np.array_equal(o.cpu().numpy(), outs[t][0]) and np.array_equal(r.cpu().numpy(), outs[t][1]), t
        assert np.array_equal(info["scenario_index"].cpu().numpy(), outs[t][2]), t
        obs = o
    other = make(start=1)
    other.reset()
    with pytest.raises(ValueError, match="scenario assignment|other scenarios"):
        other.set_state(st)
    env.close()
    env2.close()
    other.close()
