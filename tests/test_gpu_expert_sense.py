"""md_expert_sense on the MI355X (the expert observing through its own sensors, metadrive_ped_amd/expert.py): every row of
expert(env, own_sensors=True) bit for bit against the CPU oracle run with the expert's sensor config on the same scenes -- or zeros
where the env is about to restore itself -- for vehicle configs that share nothing with the expert's, capacities past 64 slots, the
PG walk and multi-agent envs whose tiles straddle envs; ExpertPolicy rollouts with the key against the oracle; batch invariance."""
import copy

import numpy as np
import pytest

import expert_host as eh

pytestmark = pytest.mark.gpu

OTHER_SENSORS = dict(random_agent_model=True,
                     vehicle_config=dict(lidar=dict(num_lasers=72, distance=40, num_others=2, gaussian_noise=0.05),
                                         side_detector=dict(num_lasers=12), lane_line_detector=dict(num_lasers=4)))
LIDAR_72 = dict(vehicle_config=dict(lidar=dict(num_lasers=72, distance=40)))


def _correct(raw):
    x = np.array(raw, np.float32, copy=True)
    x[:, 15] = np.float32(1.0) - x[:, 15]
    x[:, 10] = np.float32(1.0) - x[:, 10]
    return x


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _bad_rows(got, want):
    return np.nonzero((np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)).any(1))[0]


@pytest.fixture(scope="module")
def weights():
    return eh.packed_weights()


def _engine(user):
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    return BatchedEngine(make_config(dict(user, expert_weights=eh.WEIGHTS)))


def expert_sensor_config(cfg, cap):
    """The finished config `cfg` with the expert's own sensors (numpy_expert.py:39-46) for the vehicle's: every scene-affecting key
    stays, so the scenes are the same and the oracle's obs row is the expert's raw observation (behind [length, width] with
    random_agent_model)."""
    c = copy.deepcopy(cfg)
    vc = c["vehicle_config"]
    vc["lidar"].update(num_lasers=240, distance=50, num_others=4, gaussian_noise=0.0, dropout_prob=0.0, add_others_navi=False)
    for det in ("side_detector", "lane_line_detector"):
        vc[det].update(num_lasers=0, gaussian_noise=0.0, dropout_prob=0.0)
    c["mover_capacity"] = cap
    return c


def expert_oracle(eng, cls=None):
    """An oracle world on the engine's scenes whose vehicles carry the expert's sensors."""
    import oracle_binding as ob
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(expert_sensor_config(eng.cfg, eng.cap))
    assert host.obs_dim == 275 + (2 if eng.cfg["random_agent_model"] else 0) and host.seeds == eng.host.seeds and host.cap == eng.cap
    for k in ("shape0", "dyn0", "nav0", "param"):
        assert np.array_equal(host.state[k].view(np.uint8), eng.host.state[k].view(np.uint8)), k
    return (cls or ob.OracleWorld)(host)


def expected(orc, weights):
    """-> (corrected rows [E * A, 275], deterministic actions [E * A, 2], mlp [E * A, 4], rows not sensed): the oracle's, or zeros
    where the env is about to restore itself.  Every row has an expectation."""
    h = orc.host
    rows = orc.obs.reshape(h.E * h.A, -1)
    base = 2 if h.cfg["random_agent_model"] else 0
    assert rows.shape[1] == base + 275
    x = _correct(rows[:, base:base + 275])
    off = np.repeat(orc.state["need_reset"] != 0, h.A)
    x[off] = 0.0
    out = eh.mlp(weights, x)
    out[off] = 0.0
    return x, out[:, :2].copy(), out, off


def check_rows(env, orc, weights, where):
    from metadrive_ped_amd.expert import expert
    act, obs = expert(env, deterministic=True, need_obs=True, own_sensors=True)
    want_x, want_a, _, off = expected(orc, weights)
    got_x, got_a = obs.cpu().numpy().reshape(-1, 275), act.cpu().numpy().reshape(-1, 2)
    assert _bits_equal(got_x, want_x), "{}: expert obs differs in rows {}".format(where, _bad_rows(got_x, want_x))
    assert _bits_equal(got_a, want_a), "{}: action differs in rows {}".format(where, _bad_rows(got_a, want_a))
    return act, obs, off


@pytest.mark.parametrize("kernel", ["wg", "wave"])
def test_matched_config_equals_the_obs_row_expert(cs_dist, kernel):
    """the default vehicle config: the own-sensors expert equals the obs-row expert in obs and action on every row of an env that
    goes on, and is zero on the envs about to restore themselves"""
    import torch
    from helpers import scripted_actions
    from metadrive_ped_amd.expert import expert
    E = 16
    eng = _engine(dict(num_envs=E, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.1, start_seed=3, horizon=80,
                       step_kernel=kernel))
    eng.reset()
    resets = 0
    for t in range(300):
        a1, o1 = expert(eng, deterministic=True, need_obs=True)
        a2, o2 = expert(eng, deterministic=True, need_obs=True, own_sensors=True)
        off = eng.need_reset.cpu().numpy() != 0
        a1, o1 = a1.cpu().numpy(), o1.cpu().numpy()
        a1[off], o1[off] = 0.0, 0.0
        assert tuple(a2.shape) == (E, 2) and tuple(o2.shape) == (E, 275)
        assert _bits_equal(o2.cpu().numpy(), o1), "step {}: rows {}".format(t, _bad_rows(o2.cpu().numpy(), o1))
        assert _bits_equal(a2.cpu().numpy(), a1), t
        resets += int(off.sum())
        eng.step(torch.from_numpy(scripted_actions(E, 1, t, seed=5)).to(eng.device))
    assert resets >= E, resets


def test_everything_differs_and_the_expert_writes_no_state(cs_dist, weights):
    """17 envs (one tile plus one row) whose own observation shares nothing with the expert's: 72 beams at 40 m with num_others=2
    and noise, side and lane-line detectors, random_agent_model.  Obs and action against the oracle; the env's obs and state stay
    bit-equal to a twin engine that never calls the expert."""
    import torch
    from helpers import assert_state_equal, scripted_actions
    E = 17
    user = dict(OTHER_SENSORS, num_envs=E, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.1, start_seed=3, horizon=80)
    eng, twin = _engine(user), _engine(user)
    orc = expert_oracle(eng)
    assert eng.obs_dim != 259 and eng.n_beams == 72
    eng.reset()
    twin.reset()
    orc.reset()
    seen_off = 0
    for t in range(200):
        _, _, off = check_rows(eng, orc, weights, "step %d" % t)
        seen_off += int(off.sum())
        a = scripted_actions(E, 1, t, seed=5)
        for x in (eng, twin):
            x.step(torch.from_numpy(a).to(x.device))
        orc.step(a)
        if t % 50 == 49:
            assert_state_equal(eng.download_state(), twin.download_state(), keys=list(eng.host.state), where="twin, step %d" % t)
    assert seen_off >= E, seen_off


def test_two_lidar_chunks(cs_dist, weights):
    """72 slots and dense traffic with accident scenes: the cast walks two 64-slot chunks and the high word of the detected set
    names bodies in slots >= 64"""
    import torch
    from helpers import scripted_actions
    from metadrive_ped_amd import abi
    E = 8
    eng = _engine(dict(num_envs=E, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.3, accident_prob=0.8, start_seed=3,
                       horizon=80, mover_capacity=72))
    orc = expert_oracle(eng)
    present = (eng.host.state["shape0"]["flags"].reshape(E, 72) & abi.F_ALIVE) != 0
    assert present[:, 64:].any(), "no body in a slot >= 64"
    eng.reset()
    orc.reset()
    for t in range(150):
        check_rows(eng, orc, weights, "step %d" % t)
        a = scripted_actions(E, 1, t, seed=5)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)


def test_walk(cs_dist, weights):
    """the PG walk: an env whose episode ended has been moved to its next map already (md_swap_draw): its rows are zeros, and the
    next episode's rows are the oracle's on the next scene"""
    import torch
    import pg_walk_host as ph
    from helpers import scripted_actions
    E = 8
    eng = _engine(dict(LIDAR_72, walk_scenarios=True, num_envs=E, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.1,
                       start_seed=3, horizon=80))
    orc = expert_oracle(eng, ph.PgWalkOracle)
    eng.reset()
    orc.reset()
    zero_rows = 0
    for t in range(260):
        _, obs, off = check_rows(eng, orc, weights, "step %d" % t)
        zero_rows += int(off.sum())
        assert not obs.cpu().numpy()[off].any()
        a = scripted_actions(E, 1, t, seed=5)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
    assert zero_rows >= E and (orc.state["walk_ep"] >= 2).all(), (zero_rows, orc.state["walk_ep"])


@pytest.mark.parametrize("which", ["roundabout", "intersection"])
def test_multi_agent_tiles_straddle_envs(weights, which):
    """roundabout, 3 envs x 6 agents (18 rows: the second tile starts inside env 2); intersection, 2 envs x 12 agents with respawns:
    every slot's row -- active, dying (a static body), free -- against the oracle's, and zeros for an env whose episode is over
    (nobody left at the horizon: the coming step restores it)"""
    import torch
    from helpers import scripted_actions
    from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentIntersectionEnv, BatchedMultiAgentRoundaboutEnv
    from metadrive_ped_amd.expert import expert
    cls, E, A = dict(roundabout=(BatchedMultiAgentRoundaboutEnv, 3, 6), intersection=(BatchedMultiAgentIntersectionEnv, 2, 12))[which]
    env = cls(dict(num_envs=E, num_agents=A, horizon=80, start_seed=3, expert_weights=eh.WEIGHTS))
    env.reset()
    eng = env.engine
    orc = expert_oracle(eng)
    orc.reset()
    assert tuple(expert(env, own_sensors=True).shape) == (E, A, 2)
    seen = set()
    for t in range(300):
        act, obs, off = check_rows(env, orc, weights, "%s step %d" % (which, t))
        assert tuple(act.shape) == (E, A, 2) and tuple(obs.shape) == (E, A, 275)
        fl = orc.state["shape"]["flags"].reshape(E, -1)[:, :A]
        seen |= set(np.unique(fl & (0x10 | 0x80)).tolist())        # MD_F_ALIVE, MD_F_STATIC
        a = scripted_actions(E, A, t, seed=5)
        env.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
    assert {0x10, 0x90} <= seen, seen        # active and dying slots were among the rows


def _rollout_parity(env, weights, steps):
    """agent_policy=ExpertPolicy with expert_own_sensors: the env's oracle, stepped with the applied actions, stays bit-exact; every
    applied action is the host expert's on the expected row with the engine's draw (zeros for an env about to restore itself)."""
    import torch
    import oracle_binding as ob
    from helpers import assert_state_equal
    env.reset()
    eng = env.engine
    E, A = eng.E, eng.A
    assert "detected" not in eng.state_dev or eng.host.num_others > 0
    orc_env = ob.OracleWorld(eng.host)
    orc_env.reset()
    orc = expert_oracle(eng)
    orc.reset()
    g = torch.Generator(device=eng.device)
    g.manual_seed(int(env.config["start_seed"]))
    ended = 0
    for t in range(steps):
        _, _, out, off = expected(orc, weights)
        noise = torch.randn((E * A, 2), dtype=torch.float32, device=eng.device, generator=g).cpu().numpy()
        want = eh.sample(out, noise)
        want[off] = 0.0
        ended += int(off.sum())
        _, _, _, _, info = env.step(None)
        applied = eng._expert_action.cpu().numpy().reshape(E * A, 2)
        assert _bits_equal(applied, want), "step {}: rows {}".format(t, _bad_rows(applied, want))
        orc_env.step(applied.reshape(E, A, 2))
        orc.step(applied.reshape(E, A, 2))
        sanitised = orc_env.state["action"].reshape(E, -1, 2)[:, :A]
        assert _bits_equal(info["action"].cpu().numpy().reshape(E, A, 2), sanitised), t
        if t % 50 == 49:
            assert_state_equal(eng.download_state(), orc_env.state, where="ExpertPolicy (own sensors) step %d" % t)
    return ended


def test_expert_policy_rollout_parity_single_agent(cs_dist, weights):
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(LIDAR_72, num_envs=16, num_scenarios=16, start_seed=5, block_dist_config=cs_dist, traffic_density=0.1,
                                   horizon=80, agent_policy="ExpertPolicy", expert_own_sensors=True, expert_weights=eh.WEIGHTS))
    assert env.observation_space.shape == (19 + 72, )
    assert _rollout_parity(env, weights, 300) >= 16


def test_expert_policy_rollout_parity_roundabout(weights):
    from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentRoundaboutEnv
    env = BatchedMultiAgentRoundaboutEnv(dict(num_envs=3, num_agents=6, horizon=80, start_seed=5, agent_policy="ExpertPolicy",
                                              expert_own_sensors=True, expert_weights=eh.WEIGHTS))
    _rollout_parity(env, weights, 300)


def test_batch_invariance(cs_dist):
    """each row's bits are the same in batches of 1, 7 and 64 envs and in a second call"""
    import torch
    from helpers import scripted_actions
    from metadrive_ped_amd.expert import expert

    def run_to(E):
        eng = _engine(dict(LIDAR_72, num_envs=E, num_scenarios=8, block_dist_config=cs_dist, traffic_density=0.1, start_seed=11))
        eng.reset()
        for t in range(30):
            eng.step(torch.from_numpy(scripted_actions(64, 1, t, seed=7)[:E]).to(eng.device))
        return eng

    big = run_to(64)
    act, obs = expert(big, deterministic=True, need_obs=True, own_sensors=True)
    act, obs = act.cpu().numpy(), obs.cpu().numpy()
    assert np.isfinite(obs).all() and obs[:, 35:].min() < 1.0          # somebody's lidar sees something
    a2, o2 = expert(big, deterministic=True, need_obs=True, own_sensors=True)
    assert _bits_equal(a2.cpu().numpy(), act) and _bits_equal(o2.cpu().numpy(), obs)
    for E in (1, 7):
        small = run_to(E)
        a3, o3 = expert(small, deterministic=True, need_obs=True, own_sensors=True)
        assert _bits_equal(o3.cpu().numpy(), obs[:E]), E
        assert _bits_equal(a3.cpu().numpy(), act[:E]), E
