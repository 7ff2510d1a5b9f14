"""The scenario walk (walk_scenarios): envs that reset themselves move on through the dataset slice, one scene pool built once.

CPU: the schedule of include/md_scenario.h (md_walk_scene, through tests/walk_host.c) against the reference's
_reset_global_seed rule and the host's restatement; the oracle stepped with the host-side form of md_swap_draw
(tests/walk_host.py): every walked episode is bit-identical to a fresh one-env batch of its scenario; a checkpoint taken mid-walk
resumes exactly; a pool that does not fit is refused."""
import numpy as np
import pytest

import oracle_binding as ob
import walk_host as wh
from metadrive_ped_amd import abi
from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config, synthetic_scenarios, walk_scene

T_FRAMES = 90


def reference_seeds(start, num_scenarios, worker_index, num_workers, n):
    """ScenarioEnv._reset_global_seed with sequential_seed (envs/scenario_env.py:359-380), n resets of one worker"""
    out, current = [], None
    for _ in range(n):
        if current is None:
            current = start + worker_index
        else:
            current += num_workers
        if current >= start + num_scenarios:
            current = start + worker_index
        out.append(current)
    return out


def _walk_cfg(E, n, **kw):
    return make_scenario_config(dict(dict(num_envs=E, num_scenarios=n, walk_scenarios=True, sequential_seed=True), **kw))


@pytest.mark.parametrize("E,n,offset,stride", [(4, 10, 0, None), (4, 3, 0, None), (5, 13, 3, None), (3, 7, 9, 12),
                                               (8, 8, 0, None), (1, 4, 2, 3), (6, 20, 6, 24)])
def test_sequential_schedule_is_the_reference_multi_worker_rule(E, n, offset, stride):
    start = 17
    cfg = _walk_cfg(E, n, start_scenario_index=start, env_seed_offset=offset, walk_stride=stride)
    W = stride or E
    eps = 3 * n + 2
    e = np.repeat(np.arange(E), eps)
    ep = np.tile(np.arange(eps), E)
    dev = wh.cfg_walk_scene(cfg, e, ep).reshape(E, eps)
    assert np.array_equal(dev, walk_scene(cfg, e, ep).reshape(E, eps))     # the host's restatement
    for k in range(E):
        want = reference_seeds(start, n, (offset + k) % n, W, eps)
        assert (start + dev[k]).tolist() == want
        # worker w plays only w + j * W
        assert (((dev[k] - (offset + k) % n) % W) == 0).all()


def test_uniform_draws_are_keyed_by_env_and_episode_and_cover_the_slice():
    cfg = _walk_cfg(16, 11, sequential_seed=False, start_seed=5, env_seed_offset=32)
    e = np.repeat(np.arange(16), 40)
    ep = np.tile(np.arange(40), 16)
    a = wh.cfg_walk_scene(cfg, e, ep)
    assert np.array_equal(a, walk_scene(cfg, e, ep))
    assert a.min() >= 0 and a.max() < 11 and len(np.unique(a)) == 11
    counts = np.bincount(a, minlength=11)
    assert counts.min() > 0.5 * counts.mean()
    # another shard (offset) or another seed walks differently
    assert not np.array_equal(a, wh.cfg_walk_scene(dict(cfg, env_seed_offset=48), e, ep))
    assert not np.array_equal(a, wh.cfg_walk_scene(dict(cfg, start_seed=6), e, ep))


def test_shards_split_the_slice_like_workers():
    from metadrive_ped_amd.sharding import shard_config
    cfg = _walk_cfg(4, 24)
    seen = []
    for r in range(3):
        c = shard_config(cfg, r, 3)
        assert c["walk_stride"] == 12
        seen.append(wh.cfg_walk_scene(c, np.repeat(np.arange(4), 2), np.tile(np.arange(2), 4)))
    allp = np.concatenate(seen)
    assert sorted(allp.tolist()) == list(range(24))         # 12 workers x 2 episodes: every scenario once


def _follow(obs, n_side=12):
    o_navi = (n_side or 2) + 6 + 1
    a = np.zeros((len(obs), 1, 2), np.float32)
    a[:, 0, 0] = np.clip(6.0 * (obs[:, o_navi + 19] - 0.5) + 2.0 * (obs[:, o_navi + 18] - 0.5), -1, 1)
    a[:, 0, 1] = 0.3
    return a


def _episodes(o, E, n_steps):
    """per env: list of episodes, each a list of (obs, reward, cost, done word) rows from its reset step on"""
    eps = [[[]] for _ in range(E)]

    def rec():
        for e in range(E):
            eps[e][-1].append((o.state["obs"][e].copy(), o.state["reward"][e], o.state["cost"][e],
                               o.state["done_out"][e].copy()))
    rec()
    for _ in range(n_steps):
        ended = o.state["need_reset"].copy()
        for e in np.nonzero(ended)[0]:
            eps[e].append([])
        o.step(_follow(o.obs))
        rec()
    return eps


def _fresh_episode(pool_sc, p, cap, length, reactive):
    cfg = make_scenario_config(dict(num_envs=1, num_scenarios=1, horizon=_HORIZON, reactive_traffic=reactive, mover_capacity=cap,
                                    start_scenario_index=p))
    host = ScenarioHostScene(cfg, [pool_sc[p]])
    o = ob.OracleWorld(host)
    o.set_tracks(host.tracks["shape"], host.tracks["dyn"])
    o.reset()
    out = [(o.state["obs"][0].copy(), o.state["reward"][0], o.state["cost"][0], o.state["done_out"][0].copy())]
    for _ in range(length - 1):
        o.step(_follow(o.obs))
        out.append((o.state["obs"][0].copy(), o.state["reward"][0], o.state["cost"][0], o.state["done_out"][0].copy()))
    return out


_HORIZON = 24


@pytest.mark.parametrize("seq,E,n,reactive", [(True, 3, 5, True), (True, 4, 2, False), (False, 3, 4, True)])
def test_walked_episodes_are_fresh_episodes_on_the_oracle(seq, E, n, reactive):
    pool = synthetic_scenarios(n, 500, T=T_FRAMES)
    cfg = _walk_cfg(E, n, sequential_seed=seq, horizon=_HORIZON, reactive_traffic=reactive, start_seed=3)
    host = ScenarioHostScene(cfg, pool)
    assert host.T == T_FRAMES and len(host.map_tables) == n
    o = wh.WalkOracle(host)
    o.reset()
    eps = _episodes(o, E, 4 * (_HORIZON + 1) + 3)
    fresh = {}
    for e in range(E):
        closed = eps[e][:-1]
        assert len(closed) >= 3
        for k, ep in enumerate(closed):
            p = int(wh.cfg_walk_scene(cfg, e, k))
            if (p, len(ep)) not in fresh:
                fresh[(p, len(ep))] = _fresh_episode(pool, p, host.cap, len(ep), reactive)
            want = fresh[(p, len(ep))]
            for t, (a, b) in enumerate(zip(ep, want)):
                assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (e, k, p, t, "obs")
                assert a[1].view(np.uint32) == b[1].view(np.uint32) and a[2].view(np.uint32) == b[2].view(np.uint32), (e, k, t)
                assert np.array_equal(a[3], b[3]), (e, k, t, "done")
            assert ep[-1][3][0] or ep[-1][3][1]       # the episode ended
        assert o.state["walk_ep"][e] == len(eps[e]) - 1
        assert o.state["scene_of"][e] == wh.cfg_walk_scene(cfg, e, o.state["walk_ep"][e])
        assert o.env_map[e] == o.state["scene_of"][e]


def test_checkpoint_mid_walk_resumes_identically_on_the_oracle():
    pool = synthetic_scenarios(5, 520, T=T_FRAMES)
    cfg = _walk_cfg(3, 5, sequential_seed=False, horizon=20, reactive_traffic=True)
    host = ScenarioHostScene(cfg, pool)
    o = wh.WalkOracle(host)
    o.reset()
    for _ in range(47):
        o.step(_follow(o.obs))
    assert (o.state["walk_ep"] >= 2).all()
    saved = {k: v.copy() for k, v in o.state.items()}
    o2 = wh.WalkOracle(host, state=saved)
    o2.env_map[:] = saved["scene_of"]          # what set_state re-derives MdWorld.env_map from
    o2.w.env_map = o2.env_map.ctypes.data
    for _ in range(40):
        o.step(_follow(o.obs))
        o2.step(_follow(o2.obs))
    for k in o.state:
        assert np.array_equal(o.state[k].view(np.uint8), o2.state[k].view(np.uint8)), k


def test_pool_is_built_once_and_sized_by_the_whole_pool():
    pool = synthetic_scenarios(3, 600, T=T_FRAMES)
    longer = synthetic_scenarios(1, 602, T=T_FRAMES + 30, n_vehicles=30)[0]
    pool[2] = longer
    cfg = _walk_cfg(8, 3)
    host = ScenarioHostScene(cfg, pool)
    # T and the capacity are the pool's maxima
    assert host.T == T_FRAMES + 30
    assert host.cap >= len(longer["tracks"]) > len(pool[0]["tracks"])
    assert host.world.arrays["ckpt_off"].shape == (4, )                     # one checkpoint list per SCENE, not per env
    assert host.tracks["shape"].shape[1] == 3 * host.cap
    assert host.seeds == [0, 1, 2]
    assert host.state["scene_of"].tolist() == [e % 3 for e in range(8)]
    assert list(host.world.arrays["env_map"]) == [e % 3 for e in range(8)]
    cap = host.cap
    for e in range(8):
        p = e % 3
        assert np.array_equal(host.state["shape0"][e * cap:(e + 1) * cap], host.pool["shape0"][p * cap:(p + 1) * cap])
    assert host.walk_params == (3, 1, 8, 0, 0)


def test_walk_refuses_a_pool_that_does_not_fit():
    pool = synthetic_scenarios(4, 700, T=T_FRAMES)
    cfg = _walk_cfg(2, 4, scenario_pool_max_bytes=1 << 18)
    with pytest.raises(ValueError, match="num_scenarios=4"):
        ScenarioHostScene(cfg, pool)
    with pytest.raises(ValueError, match="num_scenarios"):
        ScenarioHostScene(_walk_cfg(2, 5), pool)      # the pool is the whole slice


def test_walk_off_is_todays_batch():
    sc = synthetic_scenarios(3, 800, T=T_FRAMES)
    a = ScenarioHostScene(make_scenario_config(dict(num_envs=3, num_scenarios=3)), sc)
    assert a.pool is None and "scene_of" not in a.state and "walk_ep" not in a.state
    assert a.walk_params == (0, 0, 0, 0, 0)
    assert list(a.world.arrays["env_map"]) == [0, 1, 2]
    assert abi.MD_ABI_VERSION == 12
