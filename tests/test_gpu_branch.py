"""Device-side env snapshots on the MI355X (md_branch, include/md_branch.h): env.snapshot() / restore() / branch() against the host
checkpoint path, against the CPU oracle stepped from branch.apply_host of the downloaded state, and against a control batch that was
only stepped; the multi-agent, top-down and AIProtect extras; one launch per call."""
import numpy as np
import pytest

from helpers import assert_state_equal, scripted_actions

pytestmark = pytest.mark.gpu

PG = dict(num_envs=8, num_scenarios=8, map="SCX", traffic_density=0.15, horizon=30)


def _pg_env(steps=12, **kw):
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(PG, **kw))
    env.reset()
    for t in range(steps):
        env.step(scripted_actions(env.num_envs, 1, t)[:, 0])
    return env


def _outputs(res):
    obs, reward, terminated, truncated, _ = res
    return [x.cpu().numpy().copy() for x in (obs, reward, terminated, truncated)]


def _run(env, t0, n, one_row=False):
    """n scripted steps from step number t0 -> [(outputs, downloaded state)] per step"""
    out = []
    for t in range(t0, t0 + n):
        a = scripted_actions(1, 1, t)[0, 0] if one_row else scripted_actions(env.num_envs, 1, t)[:, 0]
        out.append((_outputs(env.step(a)), env.engine.download_state()))
    return out


def _same_runs(a, b, where):
    assert len(a) == len(b)
    for t, ((oa, sa), (ob_, sb)) in enumerate(zip(a, b)):
        for x, y in zip(oa, ob_):
            assert x.tobytes() == y.tobytes(), (where, t)
        assert_state_equal(sa, sb, keys=list(sa), where="%s, step %d" % (where, t))


def _oracle(env, state, env_map):
    """The CPU oracle on the env's tables, from `state`, with its own env_map"""
    import oracle_binding as ob
    o = ob.OracleWorld(env.engine.host, state=state)
    o._env_map = np.ascontiguousarray(env_map, np.int32)
    o.w.env_map = o._env_map.ctypes.data
    return o


def _env_map(env):
    return env.engine.world_dev["env_map"].view(env.engine.torch.int32).cpu().numpy().copy()


def test_round_trip_equals_the_host_checkpoint_path():
    env = _pg_env()
    snap = env.snapshot()
    ck = env.get_state()
    assert snap.num_envs == 8 and snap.source_envs == tuple(range(8)) and snap.seeds == tuple(env.current_seeds)
    assert snap.nbytes > 0 and snap.batch_signature[:5] == ("pg", env.engine.cap, 1, 259, 12)
    first = _run(env, 12, 25)
    assert any(st["need_reset"].any() for _, st in first), "the run must pass an auto-reset"
    env.restore(snap)
    _same_runs(first, _run(env, 12, 25), "after restore")
    env.set_state(ck)
    _same_runs(first, _run(env, 12, 25), "after set_state")
    # the snapshot outlives a plain reset(); a new seed rebuilds the batch and invalidates it
    env.reset()
    env.restore(snap)
    _same_runs(first[:3], _run(env, 12, 3), "after reset() and restore")
    env.reset(seed=env.config["start_seed"] + 100)
    with pytest.raises(ValueError) as err:
        env.restore(snap)
    assert "no longer valid" in str(err.value)


def test_cross_env_branch_equals_the_oracle():
    from metadrive_ped_amd import branch
    env = _pg_env()
    eng = env.engine
    before, ck = eng.download_state(), env.get_state()
    env_map = _env_map(env)
    seeds = list(env.current_seeds)
    assert len(set(env_map.tolist())) == 8 and len(set(seeds)) == 8
    pairs = [(3, d) for d in (0, 1, 2, 4, 5, 6, 7)]
    env.branch(3, [d for _, d in pairs])
    branch.apply_host(before, env_map, pairs)
    assert_state_equal(eng.download_state(), before, keys=list(before), where="after branch")
    assert _env_map(env).tolist() == env_map.tolist() == [env_map[3]] * 8
    assert list(env.current_seeds) == [seeds[3]] * 8
    assert env.get_state()["__seeds__"].tolist() == [seeds[3]] * 8
    with pytest.raises(ValueError):      # a checkpoint from before the branch: another scenario assignment
        env.set_state(ck)
    orc = _oracle(env, before, env_map)
    resets = 0
    for t in range(12, 12 + 45):
        a = np.broadcast_to(scripted_actions(1, 1, t), (8, 1, 2)).copy()
        res = env.step(a[:, 0])
        orc.step(a)
        st = eng.download_state()
        assert_state_equal(st, orc.state, keys=list(st), where="branched, step %d" % t)
        resets += int(st["need_reset"].any())
        for x in _outputs(res):
            assert all(x[e].tobytes() == x[3].tobytes() for e in range(8)), t
        assert res[4]["env_seed"].cpu().numpy().tolist() == [seeds[3]] * 8
    assert resets >= 1
    env.reset()      # without a new seed the branched assignment stays: the reset snapshot rows travelled too
    obs = env.engine.obs.cpu().numpy()
    assert all(obs[e].tobytes() == obs[3].tobytes() for e in range(8)) and list(env.current_seeds) == [seeds[3]] * 8


def test_partial_restore_leaves_the_rest_alone():
    from metadrive_ped_amd import branch
    env, control = _pg_env(), _pg_env()
    at_snap = env.engine.download_state()
    map_at_snap = _env_map(env)
    snap = env.snapshot([1, 6])
    assert snap.num_envs == 2 and snap.seeds == (env.current_seeds[1], env.current_seeds[6])
    _run(env, 12, 10)
    _run(control, 12, 10)
    env.restore(snap, envs=[5, 2])       # row 0 (env 1) -> env 5, row 1 (env 6) -> env 2: odd and even row bases
    want, env_map = control.engine.download_state(), _env_map(control)
    src = {k: v.view(np.uint8).reshape(8, -1)[[1, 6]].copy() for k, v in at_snap.items()}
    src["need_reset"] = np.ascontiguousarray(at_snap["need_reset"][[1, 6]])
    src["env_map"] = map_at_snap[[1, 6]]
    branch.apply_host(want, env_map, [(0, 5), (1, 2)], src)
    got = env.engine.download_state()
    assert_state_equal(got, want, keys=list(got), where="after the partial restore")      # envs 0, 1, 3, 4, 6, 7: the control's
    assert _env_map(env).tolist() == env_map.tolist()
    s = control.current_seeds
    assert list(env.current_seeds) == [s[0], s[1], s[6], s[3], s[4], s[1], s[6], s[7]]
    orc = _oracle(env, want, env_map)
    for t in range(22, 42):
        a = scripted_actions(8, 1, t)
        env.step(a[:, 0])
        orc.step(a)
        st = env.engine.download_state()
        assert_state_equal(st, orc.state, keys=list(st), where="restored, step %d" % t)


def _marl_actions(E, A, t, one_row):
    """Scripted actions; agent 0 of every env steers hard at full throttle, so that it leaves the road early in its episode"""
    a = np.broadcast_to(scripted_actions(1, A, t), (E, A, 2)).copy() if one_row else scripted_actions(E, A, t)
    a[:, 0, :] = 1.0
    return a


@pytest.mark.parametrize("extra", [dict(), dict(delay_done=3)], ids=["default", "delay_done=3"])
def test_multi_agent_branch(extra):
    """The default delay_done (25 steps as a static body) leaves no time for a respawn inside a 40-step episode, so that case
    passes the env's reset only; with delay_done=3 agent 0 is respawned under new ids, which draws from MdState.rng."""
    from metadrive_ped_amd import branch
    from metadrive_ped_amd.envs import BatchedMultiAgentRoundaboutEnv
    env = BatchedMultiAgentRoundaboutEnv(dict(dict(num_envs=3, num_agents=4, horizon=40), **extra))
    env.reset()
    E, A = 3, 4
    for t in range(15):
        env.step(_marl_actions(E, A, t, False))
    before, env_map = env.engine.download_state(), _env_map(env)
    pairs = [(1, 0), (1, 2)]
    env.branch(1, [0, 2])
    assert env.snapshot().batch_signature[0] == "marl:roundabout"
    branch.apply_host(before, env_map, pairs)
    orc = _oracle(env, before, env_map)
    ids, wrapped = set(), False
    for t in range(15, 65):
        a = _marl_actions(E, A, t, True)
        env.step(a)
        orc.step(a)
        st = env.engine.download_state()
        assert_state_equal(st, orc.state, keys=list(st), where="marl, step %d" % t)
        for k in ("obs", "reward", "flags", "agent_id", "next_agent_id", "rng", "env_steps", "shape"):
            r = st[k].view(np.uint8).reshape(E, -1)
            assert np.array_equal(r[0], r[1]) and np.array_equal(r[2], r[1]), (t, k)
        ids |= set(st["agent_id"].reshape(E, -1)[1, :A].tolist())
        wrapped |= int(st["env_steps"][1]) < t - 20
    assert wrapped, "the run must pass the env's reset"
    if extra:
        assert len(ids) > A, "the run must pass a respawn (new agent ids)"


def test_top_down_history_travels():
    from metadrive_ped_amd.envs import BatchedTopDownMetaDriveEnvV2
    # distance=60: traffic inside the window within the first steps (checked with the host build of md_topdown.h)
    env = BatchedTopDownMetaDriveEnvV2(dict(num_envs=4, num_scenarios=4, map="SCX", traffic_density=0.3, resolution_size=32,
                                            frame_stack=3, frame_skip=2, distance=60))
    env.reset()
    for t in range(9):
        obs = env.step(scripted_actions(4, 1, t)[:, 0])[0]
    at_snap = obs.cpu().numpy().copy()
    hist = env.engine.topdown_history()
    assert (at_snap[..., 2] != at_snap[..., 3]).any(), "the stacked frames must differ for the history to show"
    snap = env.snapshot()
    assert snap.batch_signature[5] == (32, 3, 2, 5, 1)
    first = [env.step(scripted_actions(4, 1, t)[:, 0])[0].cpu().numpy().copy() for t in range(9, 16)]
    env.restore(snap)
    assert env.engine.topdown.cpu().numpy().tobytes() == at_snap.tobytes()      # the image itself is back ...
    for k, v in env.engine.topdown_history().items():                            # ... and so are the rings and cursors
        assert v.tobytes() == hist[k].tobytes(), k
    again = [env.step(scripted_actions(4, 1, t)[:, 0])[0].cpu().numpy().copy() for t in range(9, 16)]
    for t, (x, y) in enumerate(zip(first, again)):
        assert x.tobytes() == y.tobytes(), t
    # env -> env: the destination shows the source's stacked frames, not an empty history
    env.branch(2, [0])
    img = env.step(np.broadcast_to(scripted_actions(1, 1, 16)[0, 0], (4, 2)).copy())[0].cpu().numpy()
    assert img[0].tobytes() == img[2].tobytes()


def test_ai_protect_bytes_travel():
    import os
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    weights = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_weights.npz")
    E = 16
    env = BatchedMetaDriveEnv(dict(num_envs=E, map="C", traffic_density=0.1, num_scenarios=1, agent_policy="AIProtectPolicy",
                                   expert_weights=weights, save_level=0.5))
    env.reset()
    eng = env.engine
    rng = np.random.RandomState(5)
    acts = [np.stack([np.where(np.arange(E) % 2 == 0, 1.0, -1.0) * rng.uniform(0.3, 1.2, E), rng.uniform(0.2, 1.2, E)], 1).astype(np.float32)
            for _ in range(40)]
    noise = [rng.standard_normal((E, 2)).astype(np.float32) for _ in range(40)]

    def run(t0, t1):
        out = []
        for t in range(t0, t1):
            eng.step(torch.from_numpy(acts[t]).to(eng.device), noise=torch.from_numpy(noise[t]).to(eng.device))
            info = env._info()
            out.append([info[k].cpu().numpy().copy() for k in ("takeover", "takeover_start", "takeover_end")] +
                       [eng.state_dev[k].cpu().numpy().copy() for k in ("takeover", "expert_takeover")] + [eng._protect_action.cpu().numpy().copy()])
        return out

    head = run(0, 20)
    snap = env.snapshot()
    first = run(20, 40)
    assert any(x[0].any() for x in head + first), "the saver must take over somewhere in the run"
    env.restore(snap)
    assert env._info()["takeover"].cpu().numpy().tobytes() == head[-1][0].tobytes()      # the flag bytes of the last step before
    again = run(20, 40)
    for t, (a, b) in enumerate(zip(first, again)):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), t


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def md_branch(self, *args):
        self.calls += 1
        return self._lib.md_branch(*args)


def test_one_launch_per_call():
    env = _pg_env(steps=3)
    lib = env.engine.lib = _CountingLib(env.engine.lib)
    snap = env.snapshot()
    assert lib.calls == 1
    part = env.snapshot([4])
    assert lib.calls == 2
    env.restore(snap)
    assert lib.calls == 3
    env.restore(part, envs=[0, 1, 2])      # a one-row snapshot broadcasts
    assert lib.calls == 4
    env.branch(7, [5, 6])
    assert lib.calls == 5
    env.branch([3, 4], [5, 6])
    assert lib.calls == 6
    s = env.engine.download_state()["shape"].view(np.uint8).reshape(8, -1)
    assert np.array_equal(s[0], s[4]) and np.array_equal(s[1], s[4]) and np.array_equal(s[5], s[3]) and np.array_equal(s[6], s[4])
