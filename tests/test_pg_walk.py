"""The PG walk (walk_scenarios in the single-agent PG envs): envs that reset themselves move on through the seeds of
[start_seed, start_seed + num_scenarios), one scene pool built once.

CPU: the config keys and the refusals; the schedule (md_walk_scene through tests/walk_host.c against the host's restatement, the
uniform draw's spread, the sequential worker rule); the oracle stepped with the host-side form of md_swap_draw's PG walk
(tests/pg_walk_host.py): every walked episode is bit-identical to a fresh one-env batch built on that seed, for the plain, the safe
and the varying-dynamics env; a checkpoint taken mid-walk resumes exactly and one of another slice is refused."""
import types

import numpy as np
import pytest

import oracle_binding as ob
import pg_walk_host as ph
import walk_host as wh
from metadrive_ped_amd import abi
from metadrive_ped_amd.config import make_config
from metadrive_ped_amd.engine import HostScene
from metadrive_ped_amd.envs import (BatchedMetaDriveEnv, BatchedMultiAgentMetaDrive, BatchedMultiAgentRoundaboutEnv,
                                    BatchedSafeMetaDriveEnv, BatchedVaryingDynamicsEnv)
from metadrive_ped_amd.scenario import walk_params, walk_scene

WALK = dict(walk_scenarios=True, num_envs=4, num_scenarios=12)


# -- 1. config -------------------------------------------------------------------------------------------------------------------
def test_walk_config_constructs_in_the_three_single_agent_envs():
    for cls in (BatchedMetaDriveEnv, BatchedSafeMetaDriveEnv, BatchedVaryingDynamicsEnv):
        env = cls(dict(WALK))
        assert env.config["walk_scenarios"] is True and env.config["walk_stride"] is None and env.config["sequential_seed"] is False
        assert walk_params(env.config) == (12, 2, 4, 0, 0)
    cfg = BatchedMetaDriveEnv(dict(WALK, sequential_seed=True, walk_stride=16, env_seed_offset=8, start_seed=7)).config
    assert walk_params(cfg) == (12, 1, 16, 8, 7)


@pytest.mark.parametrize("extra,exc,match", [
    (dict(random_traffic=True), NotImplementedError, "random_traffic"),
    (dict(traffic_mode="replay"), NotImplementedError, "replay"),
    (dict(auto_reset=False), ValueError, "auto_reset"),
    (dict(walk_stride=0), ValueError, "walk_stride"),
])
def test_walk_refusals_by_name(extra, exc, match):
    with pytest.raises(exc, match=match):
        BatchedMetaDriveEnv(dict(WALK, **extra))


@pytest.mark.parametrize("cls", [BatchedMultiAgentMetaDrive, BatchedMultiAgentRoundaboutEnv])
def test_walk_is_refused_in_the_multi_agent_envs(cls):
    with pytest.raises(NotImplementedError, match="walk_scenarios=True in a multi-agent env"):
        cls(dict(walk_scenarios=True, num_envs=2, num_scenarios=2))


def test_recorded_traffic_is_refused_while_walking():
    """load_tracks / load_scenarios name the walk in their own message (start_recording needs an engine: tests/test_gpu_pg_walk.py)"""
    env = BatchedMetaDriveEnv(dict(WALK))
    with pytest.raises(NotImplementedError, match="load_tracks with walk_scenarios=True"):
        env.load_tracks(dict())
    with pytest.raises(NotImplementedError, match="load_scenarios with walk_scenarios=True"):
        env.load_scenarios([])
    assert env.engine is None                     # refused before anything is built
    plain = BatchedMetaDriveEnv(dict(WALK, walk_scenarios=False))
    with pytest.raises(ValueError, match="load_tracks needs config traffic_mode='replay'"):    # as before
        plain.load_tracks(dict())


def test_walk_off_is_todays_batch():
    base = dict(num_envs=5, num_scenarios=3, env_seed_offset=2, start_seed=40, map=2)
    a, b = make_config(dict(base)), make_config(dict(base, walk_scenarios=False))
    new = ("walk_scenarios", "walk_stride", "sequential_seed", "scenario_pool_max_bytes")
    assert {k: v for k, v in a.items() if k != "block_dist_config"} == {k: v for k, v in b.items() if k != "block_dist_config"}
    assert (a["walk_scenarios"], a["walk_stride"], a["sequential_seed"]) == (False, None, False)
    assert all(k in a for k in new)
    h = HostScene(a)
    assert not h.walk and h.pool is None and h.walk_params == (0, 0, 0, 0, 0)
    assert "scene_of" not in h.state and "walk_ep" not in h.state
    assert h.seeds == [40 + (2 + e) % 3 for e in range(5)]
    assert len(h.map_tables) == 3
    assert abi.MD_ABI_VERSION == 12


def test_sub_batches_and_shards_are_workers_of_one_walk():
    from metadrive_ped_amd.envs.pipeline import SubBatchedEnvs
    from metadrive_ped_amd.sharding import shard_config
    sub = SubBatchedEnvs(BatchedMetaDriveEnv, dict(WALK, num_envs=8, sequential_seed=True), sub_batches=2)
    assert [walk_params(e.config) for e in sub.envs] == [(12, 1, 8, 0, 0), (12, 1, 8, 4, 0)]
    cfg = make_config(dict(WALK, sequential_seed=True))
    assert [walk_params(shard_config(cfg, r, 3))[2:4] for r in range(3)] == [(12, 0), (12, 4), (12, 8)]


# -- 2. schedule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq", [True, False])
def test_host_restatement_equals_md_walk_scene(seq):
    for n, W, offset in [(12, 4, 0), (12, 16, 8), (5, 8, 3), (1000, 256, 512), (7, 1, 0), (3, 3, 7)]:
        cfg = make_config(dict(walk_scenarios=True, num_envs=min(W, 8), num_scenarios=n, walk_stride=W, env_seed_offset=offset,
                               sequential_seed=seq, start_seed=9))
        e = np.repeat(np.arange(cfg["num_envs"]), 50)
        ep = np.tile(np.arange(50), cfg["num_envs"])
        got = wh.walk_scene(*walk_params(cfg), e, ep)
        assert np.array_equal(got, walk_scene(cfg, e, ep)), (n, W, offset)
        assert got.min() >= 0 and got.max() < n


def test_uniform_draws_hit_every_seed_within_5_sigma():
    cfg = make_config(dict(WALK, start_seed=3))
    n, draws = 12, 20000
    e = np.repeat(np.arange(4), draws // 4)
    ep = np.tile(np.arange(draws // 4), 4)
    counts = np.bincount(wh.walk_scene(*walk_params(cfg), e, ep), minlength=n)
    p = 1.0 / n
    sigma = np.sqrt(draws * p * (1 - p))
    assert counts.sum() == draws and len(counts) == n
    assert np.abs(counts - draws * p).max() <= 5 * sigma, counts


def test_sequential_env_visits_exactly_w_plus_kW():
    for n, W, offset, E in [(12, 4, 0, 4), (12, 8, 4, 4), (10, 4, 2, 4), (5, 8, 0, 8)]:
        cfg = make_config(dict(walk_scenarios=True, sequential_seed=True, num_envs=E, num_scenarios=n, walk_stride=W, env_seed_offset=offset))
        for e in range(E):
            w = (offset + e) % n
            visited = wh.walk_scene(*walk_params(cfg), np.full(4 * n, e), np.arange(4 * n))
            assert sorted(set(visited.tolist())) == list(range(w, n, W)), (n, W, offset, e)
            assert visited[0] == w                        # episode 0 is the assignment of a batch without the walk


def test_pool_is_every_seed_once_whatever_the_env_count():
    for E in (3, 20):      # fewer and more envs than scenarios
        cfg = make_config(dict(WALK, num_envs=E, map=2, start_seed=100, sequential_seed=True))
        h = HostScene(cfg)
        assert h.seeds == list(range(100, 112)) and len(h.map_tables) == 12 and sorted(h.scenes) == h.seeds
        cap = h.cap
        assert h.pool["shape0"].shape[0] == 12 * cap and h.state["shape0"].shape[0] == E * cap
        assert h.state["scene_of"].tolist() == [e % 12 for e in range(E)]
        assert list(h.world.arrays["env_map"]) == [e % 12 for e in range(E)]
        for e in range(E):
            p = e % 12
            for k in ("shape0", "nav0", "param", "route_roads"):
                assert np.array_equal(h.state[k][e * cap:(e + 1) * cap], h.pool[k][p * cap:(p + 1) * cap]), k
        # mover_capacity = 0 takes the pool's maximum need
        assert cap >= max(1 + sc.n_traffic + sc.n_props for sc in h.scenes.values())


def test_pool_above_the_byte_limit_is_refused():
    with pytest.raises(ValueError, match="num_scenarios=12"):
        HostScene(make_config(dict(WALK, map=2, scenario_pool_max_bytes=1 << 12)))


# -- 3 / 4. episode equivalence on the oracle ------------------------------------------------------------------------------------
HORIZON = 14


def _action(p, t):
    """the action of episode step t on scenario p: a function of both, so that a fresh batch replays it"""
    a = np.zeros((1, 2), np.float32)
    a[0, 0] = 0.25 * np.sin(0.37 * t + p)
    a[0, 1] = 0.7 if (t + p) % 5 else -0.2
    return a


def _row(o, e, cap):
    st = o.state
    return (st["obs"][e].copy(), st["reward"][e].copy(), st["cost"][e].copy(), st["done_out"][e].copy(),
            st["flags"][e * cap:(e + 1) * cap].copy(), st["step_info"][e].copy())


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def _walk_episodes(host, n_steps):
    """-> per env the list of (scene, rows) of its episodes, each from its reset step on; the oracle"""
    E, cap = host.E, host.cap
    o = ph.PgWalkOracle(host)
    o.reset()
    eps = [[(int(o.state["scene_of"][e]), [_row(o, e, cap)])] for e in range(E)]
    for _ in range(n_steps):
        ended = o.state["need_reset"].copy()
        act = np.zeros((E, 1, 2), np.float32)
        for e in range(E):
            if ended[e]:       # this step restores the env onto the scene the swap gave it (its action is discarded)
                eps[e].append((int(o.state["scene_of"][e]), []))
            else:
                act[e] = _action(eps[e][-1][0], len(eps[e][-1][1]))
        o.step(act)
        for e in range(E):
            eps[e][-1][1].append(_row(o, e, cap))
    return eps, o


def _fresh_episode(make, p, cap, length):
    """a fresh one-env batch on pool scene p, driven with the same actions"""
    host = HostScene(make(p, cap))
    o = ob.OracleWorld(host)
    o.reset()
    out = [_row(o, 0, cap)]
    for t in range(1, length):
        o.step(_action(p, t).reshape(1, 1, 2))
        out.append(_row(o, 0, cap))
    return out, host


def _check_equivalence(env_cls, extra, seq, start=20):
    user = dict(WALK, map=2, traffic_mode="trigger", traffic_density=0.1, horizon=HORIZON, start_seed=start, sequential_seed=seq, **extra)
    cfg = env_cls(user).config
    host = HostScene(cfg)
    eps, o = _walk_episodes(host, 9 * (HORIZON + 1) + 2)

    def make(p, cap):
        u = dict(user, walk_scenarios=False, num_envs=1, num_scenarios=1, start_seed=start + p, mover_capacity=cap)
        return env_cls(u).config
    fresh, seen = {}, set()
    for e in range(host.E):
        closed = eps[e][:-1]
        assert len(closed) >= 3, (e, len(closed))
        for k, (p, rows) in enumerate(closed):
            assert p == int(ph.scene(host, e, k))
            seen.add(start + p)
            if (p, len(rows)) not in fresh:
                fresh[(p, len(rows))] = _fresh_episode(make, p, host.cap, len(rows))
            want, fhost = fresh[(p, len(rows))]
            for t, (a, b) in enumerate(zip(rows, want)):
                assert _same(a, b), (e, k, p, t)
            assert rows[-1][3][0] or rows[-1][3][1]        # the episode ended
            # the scene's parameters moved with it
            assert np.array_equal(host.pool["param"][p * host.cap:(p + 1) * host.cap], fhost.state["param"])
        assert o.state["walk_ep"][e] == len(eps[e]) - 1
        assert o.state["scene_of"][e] == ph.scene(host, e, o.state["walk_ep"][e]) == o.env_map[e]
    assert len(seen) >= 8, sorted(seen)
    return host


@pytest.mark.parametrize("seq", [True, False], ids=["sequential", "uniform"])
def test_walked_episodes_are_fresh_episodes_on_the_oracle(seq):
    _check_equivalence(BatchedMetaDriveEnv, {}, seq)


@pytest.mark.parametrize("seq", [True, False], ids=["sequential", "uniform"])
def test_walked_episodes_are_fresh_episodes_safe_env(seq):
    host = _check_equivalence(BatchedSafeMetaDriveEnv, {}, seq)
    assert sum(sc.n_props for sc in host.scenes.values()) > 0                # props are part of the scenes that move
    assert len({sc.n_props for sc in host.scenes.values()}) > 1


@pytest.mark.parametrize("seq", [True, False], ids=["sequential", "uniform"])
def test_walked_episodes_are_fresh_episodes_varying_dynamics_env(seq):
    host = _check_equivalence(BatchedVaryingDynamicsEnv, {}, seq)
    agent_rows = host.pool["param"][::host.cap]
    assert len({r.tobytes() for r in agent_rows}) == 12                      # every seed its own dynamics
    # dynamics_parameters() following the walk needs the device: tests/test_gpu_pg_walk.py


def test_respawn_walk_reseeds_the_traffic_stream_per_scene():
    """respawn / hybrid: the scene's xorshift state moves with the rows, so a walked episode is a fresh one there too"""
    user = dict(WALK, map=2, traffic_mode="respawn", traffic_density=0.15, horizon=HORIZON, start_seed=5, sequential_seed=True)
    host = HostScene(make_config(user))
    assert "rng" in host.pool and len(set(host.pool["rng"].tolist())) == 12
    eps, o = _walk_episodes(host, 3 * (HORIZON + 1) + 2)
    for e in range(host.E):
        for k, (p, rows) in enumerate(eps[e][:-1]):
            want, _ = _fresh_episode(lambda p, cap: make_config(dict(user, walk_scenarios=False, num_envs=1, num_scenarios=1,
                                                                     start_seed=5 + p, mover_capacity=cap)), p, host.cap, len(rows))
            for t, (a, b) in enumerate(zip(rows, want)):
                assert _same(a, b), (e, k, p, t)


# -- 5. checkpoints --------------------------------------------------------------------------------------------------------------
def test_checkpoint_mid_walk_resumes_identically_on_the_oracle():
    cfg = make_config(dict(WALK, map=2, traffic_mode="hybrid", traffic_density=0.1, horizon=HORIZON, start_seed=2))
    host = HostScene(cfg)
    o = ph.PgWalkOracle(host)
    o.reset()
    act = lambda t: np.tile(_action(1, t).reshape(1, 1, 2), (4, 1, 1))
    for t in range(37):
        o.step(act(t))
    assert (o.state["walk_ep"] >= 2).all()
    saved = {k: v.copy() for k, v in o.state.items()}
    o2 = ph.PgWalkOracle(HostScene(cfg), state=saved)
    o2.env_map[:] = saved["scene_of"]          # what set_state re-derives MdWorld.env_map from
    for t in range(37, 80):
        o.step(act(t))
        o2.step(act(t))
    for k in o.state:
        assert np.array_equal(o.state[k].view(np.uint8), o2.state[k].view(np.uint8)), k


def test_checkpoint_of_another_slice_is_refused():
    env = BatchedMetaDriveEnv(dict(WALK, map=2, start_seed=0))
    host = HostScene(env.config)
    env.engine = types.SimpleNamespace(host=host)
    state = dict({k: v.copy() for k, v in host.state.items()}, __seeds__=np.asarray(host.seeds, np.int64))
    assert "scene_of" in env._check_checkpoint(state)
    with pytest.raises(ValueError, match="another scenario assignment"):
        env._check_checkpoint(dict(state, __seeds__=np.asarray(host.seeds, np.int64) + 1))
    with pytest.raises(ValueError, match="another scenario assignment"):
        env._check_checkpoint(dict(state, __seeds__=np.asarray(host.seeds[:4], np.int64)))     # a batch without the walk
