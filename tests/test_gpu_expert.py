"""The PPO expert on the MI355X (md_expert, metadrive_ped_amd/expert.py): the expert's observation against the CPU oracle
run with the expert's own lidar config, the MLP bit for bit against the host build of include/md_expert.h, ExpertPolicy
rollouts against the oracle, the reference's expert performance test end to end, and the stochastic draws."""
import os

import numpy as np
import pytest

import expert_host as eh

pytestmark = pytest.mark.gpu


def _correct(raw):
    x = np.array(raw, np.float32, copy=True)
    x[:, 15] = np.float32(1.0) - x[:, 15]
    x[:, 10] = np.float32(1.0) - x[:, 10]
    return x


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def weights():
    return eh.packed_weights()


def _engine(user):
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    return BatchedEngine(make_config(dict(user, expert_weights=eh.WEIGHTS)))


def _oracle_with_expert_obs(eng, user):
    """An oracle world on the engine's scenes whose lidar has num_others=4: its obs row is the expert's raw observation."""
    import oracle_binding as ob
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(make_config(dict(user, mover_capacity=eng.cap, vehicle_config=dict(lidar=dict(num_others=4)))))
    assert host.obs_dim == 275 and host.seeds == eng.host.seeds
    for k in ("shape0", "dyn0", "nav0", "param"):
        assert np.array_equal(host.state[k].view(np.uint8), eng.host.state[k].view(np.uint8)), k
    return ob.OracleWorld(host)


@pytest.mark.parametrize("kernel", ["wg", "wave"])
@pytest.mark.parametrize("draws", [False, True], ids=["fixed_traffic", "random_traffic"])
def test_expert_obs_matches_oracle(cs_dist, weights, kernel, draws):
    """expert(env, need_obs=True) is, bit for bit, the corrected observation of an oracle env with num_others=4 on the same
    scenes, over 300 steps with traffic and auto-resets; the deterministic action is the host MLP's on it, bit for bit."""
    import torch
    from helpers import scripted_actions
    from metadrive_ped_amd.engine import BatchedEngine
    from metadrive_ped_amd.expert import expert
    E = 16
    user = dict(num_envs=E, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.1, start_seed=3, horizon=80,
                step_kernel=kernel)
    if draws:
        user.update(random_traffic=True, traffic_draws=3)
    eng = _engine(user)
    orc = _oracle_with_expert_obs(eng, user)
    eng.reset()
    orc.reset()
    cap, idx, resets = eng.cap, np.zeros(E, np.int64), 0
    twins = dict(param="param0", route_nodes="route_nodes0", route_roads="route_roads0", final_lane="final_lane0")
    for t in range(300):
        act, obs = expert(eng, deterministic=True, need_obs=True)
        want = _correct(orc.obs)
        got = obs.cpu().numpy()
        assert _bits_equal(got, want), "step {}: expert obs differs in envs {}".format(
            t, np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0])
        assert _bits_equal(act.cpu().numpy(), eh.mlp(weights, want)[:, :2]), "step {}".format(t)
        a = scripted_actions(E, 1, t, seed=5)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        resets += int(orc.state["need_reset"].sum())
        if draws:
            for e in np.nonzero(orc.state["need_reset"])[0]:            # what md_swap_draw does
                idx[e] = (idx[e] + 1) % len(eng.draw_hosts_)
                src = eng.draw_hosts_[idx[e]].state
                rows = slice(e * cap, (e + 1) * cap)
                for k in BatchedEngine.DRAW_ARRAYS:
                    if k in orc.state:
                        orc.state[k][rows] = src[k][rows]
                        if k in twins and twins[k] in orc.state:
                            orc.state[twins[k]][rows] = src[k][rows]
    assert resets >= E, resets


def _run_to(E, steps, cs_dist):
    import torch
    from helpers import scripted_actions
    eng = _engine(dict(num_envs=E, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.1, start_seed=11))
    eng.reset()
    for t in range(steps):
        eng.step(torch.from_numpy(scripted_actions(E, 1, t, seed=7)).to(eng.device))
    return eng


def test_expert_mlp_bit_exact_and_batch_invariant(cs_dist, weights):
    """4096 envs: mean / log_std / action equal the host build bit for bit for every env; each env's bits are the same in
    batches of 1, 7, 64 and 4096 and in a second call."""
    import torch
    from metadrive_ped_amd.expert import expert
    big = _run_to(4096, 30, cs_dist)
    out = torch.empty((4096, 4), dtype=torch.float32, device=big.device)
    act, obs = big.expert_forward(deterministic=True, need_obs=True, mlp_out=out)
    obs_np, out_np = obs.cpu().numpy(), out.cpu().numpy()
    assert np.isfinite(out_np).all()
    host = eh.mlp(weights, obs_np)
    assert _bits_equal(out_np, host)
    assert _bits_equal(act.cpu().numpy(), host[:, :2])
    assert _bits_equal(expert(big, deterministic=True).cpu().numpy(), act.cpu().numpy())
    for E in (1, 7, 64):
        small = _run_to(E, 30, cs_dist)
        a2, o2 = expert(small, deterministic=True, need_obs=True)
        assert _bits_equal(o2.cpu().numpy(), obs_np[:E]), E
        assert _bits_equal(a2.cpu().numpy(), act.cpu().numpy()[:E]), E
    # stochastic: action = mean + exp(log_std) * noise, bit for bit against the host with the same noise
    g = torch.Generator(device=big.device)
    g.manual_seed(int(big.cfg["start_seed"]) + int(big.cfg["env_seed_offset"]))
    noise = torch.randn((4096, 2), dtype=torch.float32, device=big.device, generator=g).cpu().numpy()
    a3 = big.expert_forward(deterministic=False).cpu().numpy()
    assert _bits_equal(a3, eh.sample(host, noise))


def test_expert_against_reference_golden(weights):
    """The reference's numpy expert (tests/golden/expert_policy.npz) on the rows without other vehicles, written into the
    observation buffer of an engine: corrected obs exactly, mean / log_std within 1e-5."""
    import torch
    with np.load(os.path.join(eh.GOLDEN, "expert_policy.npz")) as f:
        g = {k: f[k] for k in ("raw", "obs", "mean", "log_std")}
    raw = g["raw"]
    keep = ~(raw[:, 19:35] != 0).any(1)
    raw = raw[keep]
    n = len(raw)
    assert n >= 64
    eng = _engine(dict(num_envs=n, num_scenarios=1, traffic_density=0.0))
    eng.reset()
    st = eng.download_state()
    st["obs"][:, :19] = raw[:, :19]
    st["obs"][:, 19:] = raw[:, 35:]
    eng.upload_state({"obs": st["obs"]})
    eng._track_detected()
    eng.state_dev["detected"].zero_()
    out = torch.empty((n, 4), dtype=torch.float32, device=eng.device)
    _, obs = eng.expert_forward(deterministic=True, need_obs=True, mlp_out=out)
    out = out.cpu().numpy()
    assert _bits_equal(obs.cpu().numpy(), g["obs"][keep])
    assert np.abs(out[:, :2] - g["mean"][keep]).max() < 1e-5
    assert np.abs(out[:, 2:] - g["log_std"][keep]).max() < 1e-5


def test_expert_policy_rollout_parity(weights):
    """BatchedMetaDriveEnv(agent_policy="ExpertPolicy"), stochastic, 16 envs x 400 steps: the oracle stepped with the actions
    the engine applied stays bit-exact; every action is the host expert's on the state the previous step left (mean +
    exp(log_std) * the engine's draw), and an env that just auto-reset is driven from its reset observation."""
    import torch
    import oracle_binding as ob
    from helpers import assert_state_equal
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
    E = 16
    env = BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=16, start_seed=5, traffic_density=0.1, horizon=120,
                                   agent_policy="ExpertPolicy", expert_weights=eh.WEIGHTS))
    obs0, _ = env.reset()
    obs0 = obs0.cpu().numpy().copy()
    eng = env.engine
    orc = ob.OracleWorld(eng.host)
    orc.reset()
    g = torch.Generator(device=eng.device)
    g.manual_seed(int(env.config["start_seed"]))
    done_at, checked = [], 0
    for t in range(400):
        _, x = eng.expert_forward(deterministic=True, need_obs=True)        # the observation the policy sees (no draw)
        x = x.cpu().numpy()
        if t >= 2 and done_at[t - 2].any():
            # ended at step t-2, restored from the snapshot during step t-1: this step's action comes from the reset state
            m = done_at[t - 2]
            assert _bits_equal(eng.obs[:, 0].cpu().numpy()[m], obs0[m]), t
            checked += int(m.sum())
        noise = torch.randn((E, 2), dtype=torch.float32, device=eng.device, generator=g).cpu().numpy()
        want = eh.sample(eh.mlp(weights, x), noise)
        _, _, term, trunc, info = env.step(None)
        applied = eng._expert_action.cpu().numpy()
        assert _bits_equal(applied, want), t
        orc.step(applied.reshape(E, 1, 2))
        done_at.append((term | trunc).cpu().numpy().copy())
        # info reports the applied (sanitised) action, as under IDMPolicy
        assert _bits_equal(info["action"].cpu().numpy(), orc.state["action"].reshape(E, -1, 2)[:, 0])
        if t % 50 == 49 or t == 399:
            assert_state_equal(eng.download_state(), orc.state, where="ExpertPolicy step %d" % t)
    assert checked > 0


@pytest.mark.parametrize("name", list(eh.PERF_CONFIGS))
def test_expert_performance_on_gpu(weights, name):
    """test_expert_performance.py with expert(env, deterministic=True) -> env.step on the GPU: every episode's reward and
    end flags equal the CPU run (host expert on the oracle) bit for bit."""
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
    from metadrive_ped_amd.expert import expert
    for lane in range(3):                   # the reference's 10 episodes repeat these three exactly (deterministic expert)
        want = eh.oracle_episode(weights, name, lane)
        cfg = dict(eh.perf_config(name, lane), expert_weights=eh.WEIGHTS)
        cfg.pop("block_dist_config")
        env = BatchedMetaDriveEnv(cfg)
        env.reset()
        total = 0.0
        for t in range(want["steps"]):
            _, r, term, trunc, info = env.step(expert(env, deterministic=True))
            total += float(r.cpu().numpy()[0])
            if bool(term[0]) or bool(trunc[0]):
                break
        fl = int(env.engine.flags[0, 0]) & 0xFFFF
        assert (t + 1, total, fl) == (want["steps"], want["reward"], want["flags"]), (name, lane)
        assert fl & abi.FL_ARRIVE_DEST


def test_expert_stochastic_draws(cs_dist):
    """Same seed -> the same actions; another start_seed -> other ones; (action - mean) / exp(log_std) over 4096 x 2 draws is
    standard normal (|mean| < 0.05, |std - 1| < 0.05)."""
    import torch
    user = dict(num_envs=4096, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.1, start_seed=21)
    a, b = _engine(user), _engine(user)
    c = _engine(dict(user, start_seed=22))
    for e in (a, b, c):
        e.reset()
    out = torch.empty((4096, 4), dtype=torch.float32, device=a.device)
    xa = a.expert_forward(mlp_out=out).cpu().numpy()
    assert _bits_equal(xa, b.expert_forward().cpu().numpy())
    assert not np.array_equal(xa, c.expert_forward().cpu().numpy())
    o = out.cpu().numpy().astype(np.float64)
    z = (xa - o[:, :2]) / np.exp(o[:, 2:])
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05, (z.mean(), z.std())
