"""The PG walk on the device: md_step + md_swap_draw (swap_draw_kernel moving PG envs through the scene pool: rows, per-slot
constants, the traffic stream, scene_of / walk_ep / env_map) bit for bit against the oracle stepped with the host-side swap
(tests/pg_walk_host.py), over at least 3 episode ends per env, in every single-agent step kernel, traffic mode and agent policy;
info["env_seed"]; dynamics_parameters(); reset(); checkpoints taken mid-walk; and a batch without the walk against the same batch
stepped as before this feature."""
import numpy as np
import pytest

import expert_host as eh
import lane_change_host as lh
import pg_walk_host as ph
from helpers import assert_state_equal, scripted_actions

pytestmark = pytest.mark.gpu

HORIZON = 20
KEYS = ["shape", "dyn", "nav", "pid", "param", "action", "flags", "obs", "reward", "cost", "step_info", "done_out", "need_reset",
        "shape0", "dyn0", "nav0", "pid0", "route_nodes", "route_roads", "final_lane", "idm_rand", "scene_of", "walk_ep"]
SPAWN_KEYS = ["rng", "route_nodes0", "route_roads0", "final_lane0"]


def _user(**kw):
    return dict(dict(walk_scenarios=True, num_envs=6, num_scenarios=10, map=2, traffic_density=0.15, horizon=HORIZON, start_seed=30), **kw)


def _env_map(eng):
    import torch
    return eng.world_dev["env_map"].view(torch.int32).cpu().numpy()


def _run_parity(user, steps=None, every=7):
    """engine against oracle, both walking; `user`: a user config, or an env's finished one; -> (engine, oracle)"""
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    cfg = user if "is_multi_agent" in user else make_config(user)
    eng = BatchedEngine(cfg)
    host, E = eng.host, cfg["num_envs"]
    policy = cfg["agent_policy"]
    lane_change = policy == "LaneChangePolicy"
    o = ph.PgWalkLaneChangeOracle(host) if lane_change else ph.PgWalkOracle(host)
    oracle = o.o if lane_change else o
    keys = KEYS + (SPAWN_KEYS if "rng" in host.state else [])

    def expected():
        ref = {k: v.copy() for k, v in oracle.state.items()}
        if lane_change:      # the agents' PID rows are the restatement's
            rows = o.agent_rows()
            for k in lh.PID_ERRS:
                ref["pid"][k][rows] = o.pid[k][rows]
        return ref

    def check(where):
        assert_state_equal(eng.download_state(), expected(), keys=keys, where=where)
        assert np.array_equal(_env_map(eng), oracle.env_map), where

    eng.reset()
    o.reset()
    check("walk reset")
    rng = np.random.RandomState(4)
    steps = steps or 4 * (HORIZON + 1) + 2
    for t in range(steps):
        if policy == "IDMPolicy":
            eng.step(None)
            o.step(None)
        elif lane_change:
            d = np.zeros((E, 1, 2), np.float32)
            d[..., 0] = rng.randint(-1, 2, (E, 1))
            d[..., 1] = rng.choice(np.float32([0.0, 0.5, 1.0]), (E, 1))
            eng.step(torch.from_numpy(d).to(eng.device))
            o.step(d)
        elif policy == "ExpertPolicy":
            eng.step(None)
            o.step(eng._expert_action.cpu().numpy().reshape(E, 1, 2))
        else:
            a = scripted_actions(E, 1, t, seed=3)
            eng.step(torch.from_numpy(a).to(eng.device))
            o.step(a)
        if t % every == 0 or t >= steps - 3:
            check("walk step %d" % t)
    st = eng.download_state()
    assert (st["walk_ep"] >= 3).all(), st["walk_ep"]
    assert np.array_equal(st["scene_of"], ph.scene(host, np.arange(E), st["walk_ep"]))
    return eng, oracle


@pytest.mark.parametrize("policy", ["EnvInputPolicy", "IDMPolicy", "LaneChangePolicy"])
@pytest.mark.parametrize("mode", ["trigger", "respawn", "hybrid"])
@pytest.mark.parametrize("kernel", ["wg", "wave"])
def test_walk_gpu_parity(kernel, mode, policy):
    extra = dict(discrete_action=True) if policy == "LaneChangePolicy" else {}
    eng, _ = _run_parity(_user(step_kernel=kernel, traffic_mode=mode, agent_policy=policy, sequential_seed=(mode != "hybrid"), **extra))
    assert eng.host.step_kernel == kernel


def test_walk_gpu_parity_default_config_takes_the_lean_kernel():
    """the reference's default MetaDriveEnv config plus the walk: trigger traffic, EnvInputPolicy, step_kernel auto -> the workgroup
    kernel's lean variant (no respawn code, no detected sets)"""
    eng, _ = _run_parity(dict(walk_scenarios=True, num_envs=6, num_scenarios=10, horizon=HORIZON))
    assert eng.host.step_kernel == "wg" and eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and "detected" not in eng.state_dev


@pytest.mark.parametrize("kernel", ["wg", "wave"])
def test_walk_gpu_parity_with_side_and_lane_line_detectors(kernel):
    """the detector clouds are launches of their own after md_step: they trace the map of the episode that ended, so the swap (which
    rewrites env_map) comes after them -- the terminal step's observation is checked at every step"""
    vc = dict(side_detector=dict(num_lasers=8, distance=50), lane_line_detector=dict(num_lasers=6, distance=20))
    eng, oracle = _run_parity(_user(step_kernel=kernel, vehicle_config=vc), every=1)
    L = eng.host.layout
    assert L.n_side == 8 and L.n_ll == 6
    maps = {len(mt.lanes) for mt in eng.host.map_tables}
    assert len(maps) > 1                       # the pool's maps differ: a cloud traced on the next scene's map would differ too


def test_walk_gpu_parity_more_envs_than_scenarios():
    eng, _ = _run_parity(_user(num_envs=40, num_scenarios=7, traffic_mode="hybrid"), every=20)
    assert len(eng.host.map_tables) == 7


def test_walk_gpu_parity_expert_policy():
    _run_parity(dict(walk_scenarios=True, num_envs=6, num_scenarios=10, horizon=HORIZON, traffic_density=0.1, start_seed=5,
                     agent_policy="ExpertPolicy", expert_weights=eh.WEIGHTS))


def test_walk_gpu_parity_safe_and_varying_dynamics_envs():
    import torch
    from metadrive_ped_amd.envs import BatchedSafeMetaDriveEnv, BatchedVaryingDynamicsEnv
    _run_parity(BatchedSafeMetaDriveEnv(_user(num_scenarios=12)).config)
    env = BatchedVaryingDynamicsEnv(_user(num_scenarios=12, sequential_seed=True))
    env.reset()
    host = env.engine.host
    keys = ("max_engine_force", "max_brake_force", "wheel_friction", "max_steering", "mass")
    moved = 0
    for t in range(3 * (HORIZON + 1)):
        env.step(torch.from_numpy(scripted_actions(6, 1, t)[:, 0]).to(env.engine.device))
        seeds = env.current_seeds.cpu().numpy()
        want = [{k: host.scenes[int(s)].vehicle_cfgs[0][k] for k in keys} for s in seeds]
        assert env.dynamics_parameters() == want, t
        moved += int((seeds != 30 + np.arange(6)).any())
    assert moved > 0
    env.close()


def test_sub_batches_walk_as_one_batch():
    """envs/pipeline.py with two sub-batches: the same walk, env for env, as one batch of the whole size"""
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    from metadrive_ped_amd.envs.pipeline import SubBatchedEnvs
    for seq in (True, False):
        user = _user(num_envs=8, sequential_seed=seq, traffic_mode="respawn")
        whole = BatchedMetaDriveEnv(user)
        sub = SubBatchedEnvs(BatchedMetaDriveEnv, user, sub_batches=2)
        whole.reset()
        sub.reset()
        for t in range(4 * (HORIZON + 1) + 2):
            a = torch.from_numpy(scripted_actions(8, 1, t)[:, 0])
            obs, r, te, tr, info = whole.step(a.to(whole.engine.device))
            parts = sub.step([a[:4], a[4:]])
            sub.synchronize()
            torch.cuda.synchronize()
            assert np.array_equal(obs.cpu().numpy().view(np.uint32), np.concatenate([p[0].cpu().numpy() for p in parts]).view(np.uint32)), t
            assert np.array_equal(info["env_seed"].cpu().numpy(), np.concatenate([p[4]["env_seed"].cpu().numpy() for p in parts])), t
        assert (whole.engine.download_state()["walk_ep"] >= 3).all()
        whole.close()
        sub.close()


def test_info_env_seed_follows_scene_of_every_step_and_reset_restarts_the_walk():
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    E, n, start = 8, 13, 40
    env = BatchedMetaDriveEnv(dict(walk_scenarios=True, num_envs=E, num_scenarios=n, start_seed=start, map=2, horizon=8))
    runs = []
    for _ in range(2):       # reset() goes back to episode 0: the same seeds again
        obs, info = env.reset()
        assert (env.engine.download_state()["walk_ep"] == 0).all()
        seen = [info["env_seed"].cpu().numpy().copy()]
        assert np.array_equal(seen[0], start + ph.scene(env.engine.host, np.arange(E), 0))
        for t in range(70):
            obs, r, term, trunc, info = env.step(torch.from_numpy(scripted_actions(E, 1, t)[:, 0]).to(env.engine.device))
            st = env.engine.download_state()
            seed = info["env_seed"]
            assert seed.is_cuda and seed.dtype == torch.int64
            assert np.array_equal(seed.cpu().numpy(), start + st["scene_of"]), t
            assert np.array_equal(info["scenario_index"].cpu().numpy(), st["scene_of"]), t
            assert np.array_equal(st["scene_of"], ph.scene(env.engine.host, np.arange(E), st["walk_ep"])), t
            assert np.array_equal(env.current_seeds.cpu().numpy(), start + st["scene_of"]) and int(env.current_seed) == start + st["scene_of"][0]
            assert np.array_equal(_env_map(env.engine), st["scene_of"]), t
            seen.append(seed.cpu().numpy().copy())
        runs.append(np.stack(seen))
    assert np.array_equal(runs[0], runs[1])
    assert len(np.unique(runs[0])) >= 8 and runs[0].min() >= start and runs[0].max() < start + n
    # reset(seed=s) re-bases the slice and rebuilds the pool
    obs, info = env.reset(seed=200)
    assert env.engine.host.seeds == list(range(200, 200 + n))
    assert np.array_equal(info["env_seed"].cpu().numpy(), 200 + ph.scene(env.engine.host, np.arange(E), 0))
    env.close()


def test_walk_checkpoint_resumes_exactly_and_refuses_another_slice():
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv

    def make(start=0, **kw):
        return BatchedMetaDriveEnv(dict(dict(walk_scenarios=True, num_envs=6, num_scenarios=10, start_seed=start, map=2, horizon=10,
                                             traffic_mode="hybrid"), **kw))

    def act(t, env):
        return torch.from_numpy(scripted_actions(6, 1, t)[:, 0]).to(env.engine.device)
    env = make()
    env.reset()
    for t in range(27):
        env.step(act(t, env))
    st = env.get_state()
    assert (st["walk_ep"] >= 2).all() and st["__seeds__"].tolist() == list(range(10))
    outs = []
    for t in range(27, 60):
        o, r, te, tr, info = env.step(act(t, env))
        outs.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), info["env_seed"].cpu().numpy().copy()))
    env2 = make()
    env2.reset()
    for t in range(5):
        env2.step(act(t, env2))
    env2.set_state(st)
    for t in range(27, 60):
        o, r, te, tr, info = env2.step(act(t, env2))
        k = t - 27
        assert np.array_equal(o.cpu().numpy().view(np.uint32), outs[k][0].view(np.uint32)), t
        assert np.array_equal(r.cpu().numpy().view(np.uint32), outs[k][1].view(np.uint32)), t
        assert np.array_equal(info["env_seed"].cpu().numpy(), outs[k][2]), t
    other = make(start=1)
    other.reset()
    with pytest.raises(ValueError, match="another scenario assignment"):
        other.set_state(st)
    assert "__env_map__" not in st and st["__walk__"].tolist() == [10, 2, 6, 0, 0]
    for kw in (dict(sequential_seed=True), dict(walk_stride=12), dict(env_seed_offset=6)):     # the same slice, another walk
        o2 = make(**kw)
        o2.reset()
        with pytest.raises(ValueError, match="another walk"):
            o2.set_state(st)
        o2.close()
    plain = make(walk_scenarios=False, num_scenarios=10, num_envs=6)
    plain.reset()
    with pytest.raises(ValueError):
        plain.set_state(st)
    for e in (env, env2, other, plain):
        e.close()


def test_start_recording_is_refused_while_walking():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(_user())
    env.reset()
    with pytest.raises(NotImplementedError, match="start_recording with walk_scenarios=True"):
        env.start_recording(10)
    assert env.engine._rec is None
    env.close()


@pytest.mark.parametrize("kernel", ["wg", "wave"])
@pytest.mark.parametrize("mode", ["trigger", "respawn"])
def test_walk_off_is_the_batch_as_before(kernel, mode):
    """walk off: no staged state, no md_swap_draw launch, and the results of the plain oracle bit for bit (the code path of a batch
    before this feature), over several auto-resets onto the same scene"""
    import torch
    import oracle_binding as ob
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    E = 12
    cfg = make_config(dict(num_envs=E, num_scenarios=5, map=2, traffic_density=0.15, horizon=HORIZON, start_seed=30, step_kernel=kernel,
                           traffic_mode=mode))
    eng = BatchedEngine(cfg)
    assert eng._staged is None and not eng._walk and eng.s.walk.mode == 0 and not eng.s.scene_of
    assert "scene_of" not in eng.state_dev
    orc = ob.OracleWorld(eng.host)
    eng.reset()
    orc.reset()
    env_map0 = _env_map(eng).copy()
    for t in range(3 * (HORIZON + 1)):
        a = scripted_actions(E, 1, t, seed=3)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        if t % 9 == 0:
            assert_state_equal(eng.download_state(), orc.state, keys=[k for k in KEYS if k in orc.state], where="step %d" % t)
    assert_state_equal(eng.download_state(), orc.state, keys=[k for k in KEYS if k in orc.state], where="end")
    assert np.array_equal(_env_map(eng), env_map0)
