"""The curriculum of the scenario walk on the device: md_step + md_curriculum (curriculum_kernel; at one level after md_swap_draw)
bit for bit against the oracle stepped with the host model of include/md_curriculum.h (tests/curriculum_host.py), on every state
array including the curriculum's; the five info keys and scenario_index; checkpoints mid-curriculum; a one-level walk is the
walk without the launch."""
import numpy as np
import pytest

import curriculum_host as ch
from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config, synthetic_scenarios

pytestmark = pytest.mark.gpu

T_FRAMES = 60
KEYS = ["shape", "dyn", "nav", "pid", "param", "action", "flags", "obs", "reward", "cost", "step_info", "need_reset", "next_agent_id",
        "shape0", "dyn0", "scene_of", "walk_ep", "cur_level", "cur_seed", "cur_q_len", "cur_q_key", "cur_q_success", "cur_q_route",
        "cur_cover", "cur_cover_n", "cur_rep_i", "cur_rep_f"]


def _actions(obs):
    """follow the route at full throttle (these envs arrive), every odd env brakes (these never do)"""
    o_navi = 12 + 6 + 1
    a = np.zeros((len(obs), 1, 2), np.float32)
    a[:, 0, 0] = np.clip(6.0 * (obs[:, o_navi + 19] - 0.5) + 2.0 * (obs[:, o_navi + 18] - 0.5), -1, 1)
    a[:, 0, 1] = 1.0
    a[1::2, 0, 1] = -1.0
    return a


def _raw(E, n, **kw):
    return dict(dict(num_envs=E, num_scenarios=n, walk_scenarios=True, sequential_seed=True, horizon=90, curriculum_level=2,
                     target_success_rate=0.5), **kw)


def _cfg(E, n, **kw):
    return make_scenario_config(_raw(E, n, **kw))


@pytest.mark.parametrize("E,n,stride,steps", [(4, 8, None, 400), (1024, 32, 16, 300)])
def test_curriculum_gpu_parity(E, n, stride, steps):
    import torch
    from helpers import assert_state_equal
    from metadrive_ped_amd.engine import BatchedEngine
    cfg = _cfg(E, n, walk_stride=stride)
    host = ScenarioHostScene(cfg, synthetic_scenarios(n, 900, T=T_FRAMES))
    eng = BatchedEngine(cfg, host=host)
    o = ch.CurriculumOracle(host)
    eng.reset()
    o.reset()
    assert_state_equal(eng.download_state(), o.state, keys=KEYS, where="curriculum reset")
    for t in range(steps):
        a = _actions(o.obs)
        eng.step(torch.from_numpy(a).to(eng.device))
        o.step(a, threads=16 if E > 64 else 1)
        if t % 25 == 0 or t == steps - 1:
            assert_state_equal(eng.download_state(), o.state, keys=KEYS, where="curriculum step %d" % t)
            assert np.array_equal(eng.world_dev["env_map"].view(torch.int32).cpu().numpy(), o.env_map), t
    lv = o.state["cur_level"]
    assert lv.max() == 1 and lv.min() == 0          # the arriving envs level up, the braking ones do not
    assert (o.state["walk_ep"] >= 2).all()


def test_curriculum_info_keys_and_checkpoint():
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    E, n = 4, 8
    cfg = _raw(E, n, start_scenario_index=3)
    pool = synthetic_scenarios(n, 900, T=T_FRAMES)
    env = BatchedScenarioEnv(cfg, scenarios=pool)
    env.reset()
    o = ch.CurriculumOracle(env.host)
    o.reset()
    diff = env.host.difficulty
    saved, env2 = None, None
    for t in range(300):
        a = _actions(o.obs)
        _, _, _, _, info = env.step(torch.from_numpy(a[:, 0, :]).to(env.engine.device))
        o.step(a)
        lvl, seed = o.state["cur_rep_i"][:, 0], o.state["cur_rep_i"][:, 1]
        assert info["curriculum_level"].cpu().numpy().tolist() == lvl.tolist(), t
        assert info["scenario_index"].cpu().numpy().tolist() == (3 + seed).tolist(), t
        assert info["scenario_difficulty"].cpu().numpy().tolist() == diff[seed].tolist(), t
        for k, i in (("curriculum_success", 0), ("curriculum_route_completion", 1), ("data_coverage", 2)):
            assert info[k].cpu().numpy().tolist() == o.state["cur_rep_f"][:, i].tolist(), (t, k)
        if t == 150:
            saved = env.get_state()
            assert saved["cur_level"].max() == 1
            env2 = BatchedScenarioEnv(cfg, scenarios=pool)
            env2.reset()
            env2.set_state(saved)
        if t > 150:
            _, _, _, _, info2 = env2.step(torch.from_numpy(a[:, 0, :]).to(env2.engine.device))
            for k in ("curriculum_level", "curriculum_success", "curriculum_route_completion", "data_coverage", "scenario_index"):
                assert torch.equal(info[k], info2[k]), (t, k)
    s1, s2 = env.get_state(), env2.get_state()
    for k in s1:
        if not k.startswith("__"):
            assert np.array_equal(s1[k].view(np.uint8), s2[k].view(np.uint8)), k


def test_one_level_walk_is_the_walk_without_the_launch():
    import torch
    from metadrive_ped_amd.engine import BatchedEngine
    E, n = 64, 16
    cfg = _cfg(E, n, curriculum_level=1, horizon=30)
    host = ScenarioHostScene(cfg, synthetic_scenarios(n, 900, T=T_FRAMES))
    a_eng = BatchedEngine(cfg, host=host)
    b_eng = BatchedEngine(cfg, host=host)
    b_eng._cur = None          # md_swap_draw alone, as before the curriculum
    a_eng.reset()
    b_eng.reset()
    for t in range(120):
        a = torch.from_numpy(_actions(a_eng.obs[:, 0, :].cpu().numpy())[:, 0, :]).to(a_eng.device)
        a_eng.step(a)
        b_eng.step(a)
    sa, sb = a_eng.download_state(), b_eng.download_state()
    for k in sa:
        if not k.startswith("cur_"):
            assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k
    assert sa["cur_cover_n"].min() >= 1 and (sa["walk_ep"] >= 1).all()
    assert sa["cur_level"].max() == 0
