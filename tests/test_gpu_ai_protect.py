"""agent_policy="AIProtectPolicy" on the MI355X (md_ai_protect, include/md_ai_protect.h): the kernel against the host build of the
header at every tile shape, the save_level extremes against ExpertPolicy and EnvInputPolicy, expert_takeover, auto-reset and
discrete actions.  Map "C", traffic_density 0.1, one scenario."""
import numpy as np
import pytest

import ai_protect_host as ah
import expert_host as eh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights():
    return eh.packed_weights()


def _env(E, policy="AIProtectPolicy", **kw):
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
    cfg = dict(num_envs=E, map="C", traffic_density=0.1, num_scenarios=1, agent_policy=policy, expert_weights=eh.WEIGHTS)
    cfg.update(kw)
    env = BatchedMetaDriveEnv(cfg)
    env.reset()
    return env


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _generator(env):
    import torch
    g = torch.Generator(device=env.engine.device)
    g.manual_seed(int(env.config["start_seed"]) + int(env.config["env_seed_offset"]))
    return g


def _noise(env, g):
    import torch
    return torch.randn((env.num_envs, 2), dtype=torch.float32, device=env.engine.device, generator=g)


def _step_with_host(env, weights, decoded, noise, step=None):
    """One env step with the host restatement beside it: the saver's draw, the applied action, the flag bytes and both state bytes
    must be the host's bit for bit.  decoded [E, 2]: the agents' decoded actions; step: what to call instead of
    engine.step(decoded, noise).  -> (step result or None, applied, flags, the saver's draw)"""
    import torch
    eng = env.engine
    E = env.num_envs
    st = eng.download_state()
    obs = eng.obs[:, 0].cpu().numpy().copy()
    _, x = eng.expert_forward(deterministic=True, need_obs=True)
    sv = eh.sample(eh.mlp(weights, x.cpu().numpy()), noise.cpu().numpy())
    tk, et = st["takeover"].copy(), st["expert_takeover"].copy()
    want_a, want_f, _ = ah.batch(eng.host.world.arrays, st, eng.host.md_config, obs, decoded, sv, env.config["save_level"], tk, et)
    if step is None:
        out = eng.step(torch.from_numpy(np.ascontiguousarray(decoded, np.float32)).to(eng.device), noise=noise)
    else:
        out = step()
    applied, flags = eng._protect_action.cpu().numpy(), eng.protect_flags.cpu().numpy()
    live = st["need_reset"] == 0          # an env that resets in this step has no saver's draw to compare
    assert np.array_equal(_bits(applied), _bits(want_a)), np.nonzero((_bits(applied) != _bits(want_a)).any(1))[0]
    assert np.array_equal(flags, want_f)
    assert np.array_equal(eng.state_dev["takeover"].cpu().numpy(), tk)
    assert np.array_equal(eng.state_dev["expert_takeover"].cpu().numpy(), et)
    assert E == len(applied)
    return out, applied, flags, sv, live


@pytest.mark.parametrize("E", [1, 15, 16, 17, 33])
def test_kernel_matches_host_at_every_batch_size(weights, E):
    """A partial tile, a full tile, one over, two tiles plus one: 30 steps of fixed pseudo-random actions and a supplied noise
    tensor; applied action, flags and state bytes equal the host restatement on the downloaded observation and state, and the
    saver's draw (saver_out) equals the host expert's."""
    import torch
    env = _env(E, save_level=0.5)
    eng = env.engine
    rng = np.random.RandomState(100 + E)
    saver = torch.empty((E, 2), dtype=torch.float32, device=eng.device)
    seen = set()
    for t in range(30):
        # every env steers towards one side and keeps the throttle up, so that the saver has work within the 30 steps
        a = np.stack([np.where(np.arange(E) % 2 == 0, 1.0, -1.0) * rng.uniform(0.3, 1.2, E), rng.uniform(0.2, 1.2, E)], 1).astype(np.float32)
        noise = torch.from_numpy(rng.standard_normal((E, 2)).astype(np.float32)).to(eng.device)
        if t % 7 == 3:      # saver_out as well
            st = eng.download_state()
            tk, et = eng.state_dev["takeover"].clone(), eng.state_dev["expert_takeover"].clone()
            eng.ai_protect_forward(torch.from_numpy(a).to(eng.device), noise=noise, saver_out=saver)
            eng.state_dev["takeover"].copy_(tk)           # the call above was a look, not the step's decision
            eng.state_dev["expert_takeover"].copy_(et)
            _, x = eng.expert_forward(deterministic=True, need_obs=True)
            assert np.array_equal(_bits(saver.cpu().numpy()), _bits(eh.sample(eh.mlp(weights, x.cpu().numpy()), noise.cpu().numpy())))
        _, applied, flags, sv, _ = _step_with_host(env, weights, a, noise)
        seen |= set(flags.tolist())
    if E >= 15:      # the comparison above had something to compare
        assert ah.TAKEOVER_START in seen, seen


def test_save_level_one_is_the_expert_from_the_second_step_on():
    """save_level = 1.0: the first step applies the agent's own action (the reference's one-step delay of the takeover flag), every
    later step applies what ExpertPolicy's kernel (md_expert) gives on the same state with the same noise, whatever the agent asks."""
    import torch
    E = 17
    env = _env(E, save_level=1.0)
    eng = env.engine
    g = _generator(env)
    rng = np.random.RandomState(7)
    for t in range(10):
        noise = _noise(env, g)
        want = eng.expert_forward(noise=noise).cpu().numpy()
        user = rng.uniform(-1.3, 1.3, (E, 2)).astype(np.float32)
        _, _, _, _, info = env.step(torch.from_numpy(user))          # the engine's own generator: the same seed, one draw per step
        applied = eng._protect_action.cpu().numpy()
        assert np.array_equal(_bits(applied), _bits(np.clip(user, -1, 1) if t == 0 else want)), t
        assert (eng.protect_flags.cpu().numpy() == (ah.TAKEOVER_START if t == 0 else ah.TAKEOVER)).all(), t
        assert bool(info["takeover"].all()) == (t > 0) and bool(info["takeover_start"].all()) == (t == 0)
        assert not bool(info["takeover_end"].any())


def test_save_level_zero_is_env_input_policy():
    """save_level = 0.0: obs, reward, done flags and flag words equal a plain EnvInputPolicy batch array for array, no flag is ever
    reported and the actions go through clipped."""
    import torch
    E = 17
    a, b = _env(E, save_level=0.0, horizon=20), _env(E, policy="EnvInputPolicy", horizon=20)
    rng = np.random.RandomState(11)
    for t in range(45):
        act = torch.from_numpy(rng.uniform(-1.3, 1.3, (E, 2)).astype(np.float32)).to(a.engine.device)
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra[:4], rb[:4]):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), t
        assert np.array_equal(a.engine.flags.cpu().numpy(), b.engine.flags.cpu().numpy()), t
        info = ra[4]
        assert not bool(info["takeover"].any() | info["takeover_start"].any() | info["takeover_end"].any())
        assert np.array_equal(_bits(info["action"].cpu().numpy()), _bits(rb[4]["action"].cpu().numpy()))


def test_set_expert_takeover(weights):
    """Envs whose expert_takeover is set follow the expert's draw with takeover False; the others keep their own action."""
    import torch
    E = 17
    env = _env(E, save_level=0.0)
    eng = env.engine
    subset = [0, 3, 16]
    env.set_expert_takeover(True, envs=subset)
    mask = np.zeros(E, bool)
    mask[subset] = True
    assert np.array_equal(env.expert_takeover.cpu().numpy(), mask)
    g = _generator(env)
    rng = np.random.RandomState(5)
    for t in range(6):
        a = rng.uniform(-1.3, 1.3, (E, 2)).astype(np.float32)
        out, applied, flags, sv, _ = _step_with_host(env, weights, a, _noise(env, g), step=lambda: env.step(torch.from_numpy(a)))
        assert np.array_equal(_bits(applied[mask]), _bits(sv[mask]))
        assert np.array_equal(_bits(applied[~mask]), _bits(np.clip(a, -1, 1)[~mask]))
        assert not flags.any() and not bool(out[4]["takeover"].any())
    env.set_expert_takeover(torch.tensor([False, True, True]), envs=subset)
    mask[0] = False
    assert np.array_equal(env.expert_takeover.cpu().numpy(), mask)
    state = env.get_state()
    assert np.array_equal(state["expert_takeover"], mask.astype(np.uint8)) and "takeover" in state
    env.set_expert_takeover(False)
    assert not bool(env.expert_takeover.any())
    env.set_state(state)
    assert np.array_equal(env.expert_takeover.cpu().numpy(), mask)
    env.reset()
    assert not bool(env.expert_takeover.any())


def test_auto_reset_clears_both_bytes(weights):
    """horizon = 5: in the step that restores an env, takeover and expert_takeover are cleared, no flag is reported and the agent's
    action passes through; the takeover then starts again."""
    import torch
    E = 17
    env = _env(E, save_level=1.0, horizon=5)
    eng = env.engine
    env.set_expert_takeover(True, envs=[2])
    g = _generator(env)
    rng = np.random.RandomState(9)
    for t in range(8):
        a = rng.uniform(-1.3, 1.3, (E, 2)).astype(np.float32)
        resets = eng.need_reset.cpu().numpy() != 0
        out, applied, flags, sv, _ = _step_with_host(env, weights, a, _noise(env, g), step=lambda: env.step(torch.from_numpy(a)))
        info = out[4]
        if t == 5:
            assert resets.all()
            assert not flags.any() and not bool(info["takeover"].any() | info["takeover_start"].any() | info["takeover_end"].any())
            assert not bool(env.expert_takeover.any()) and not eng.state_dev["takeover"].cpu().numpy().any()
            assert np.array_equal(_bits(applied), _bits(a))
        else:
            assert not resets.any()
            started = t in (0, 6)
            others = np.arange(E) != 2 if t < 5 else np.ones(E, bool)
            assert (flags[others] == (ah.TAKEOVER_START if started else ah.TAKEOVER)).all(), (t, flags)
        if t < 5:
            assert flags[2] == 0 and bool(env.expert_takeover[2])
        assert bool(out[3].all()) == (t == 4)


def test_discrete_actions(weights):
    """discrete_action = True: step() takes grid indices, the saver sees the decoded action (EnvInputPolicy.convert_to_continuous_action)."""
    import torch
    E = 16
    env = _env(E, save_level=0.5, discrete_action=True, discrete_steering_dim=5, discrete_throttle_dim=5)
    g = _generator(env)
    rng = np.random.RandomState(13)
    seen = set()
    for t in range(25):
        idx = np.where(np.arange(E) % 2 == 0, 4, 0) + 5 * rng.randint(3, 5, E)          # hard left / right, throttle 0.5 or 1
        decoded = np.stack([(idx % 5) * 0.5 - 1.0, (idx // 5) * 0.5 - 1.0], 1).astype(np.float32)
        out, applied, flags, _, _ = _step_with_host(env, weights, decoded, _noise(env, g), step=lambda: env.step(torch.from_numpy(idx)))
        seen |= set(flags.tolist())
    assert ah.TAKEOVER_START in seen, seen
