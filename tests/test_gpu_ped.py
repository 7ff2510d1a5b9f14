"""Crossing pedestrians on the MI355X (md_ped, include/md_ped.h): the engine -- md_ped before every md_step -- against the host rule
(tests/ped_host.c) applied to the CPU oracle's state before each of its steps, bit for bit in every state array and step output,
in every step-kernel variant; beside user-spawned participants; through snapshots, branch, the PG walk and random_traffic; and
the launch count.  The start seeds are the ones at which the host alone shows a kerb hold and a mid-crossing stop
(tests/test_ped_policy.py: PARITY_RUNS; found with the same host rollout)."""
import numpy as np
import pytest

import ped_host
from helpers import assert_state_equal, scripted_actions
from metadrive_ped_amd import abi
from test_ped_policy import PARITY_RUNS

pytestmark = pytest.mark.gpu

PG = dict(num_envs=8, num_scenarios=8, map="SCX", traffic_density=0.15, horizon=30, num_pedestrians=3)
STEPS = 60


class PedOracle:
    """The oracle with the pedestrians' rule in front of every step, as BatchedEngine._step_raw has it"""
    def __init__(self, host, orc=None, state=None):
        import oracle_binding as ob
        self.o = orc if orc is not None else ob.OracleWorld(host, state=state)
        self.host, self.ped, self.cover = host, abi.make_md_ped(host.cfg["pedestrian_config"]), ped_host.Coverage()
        self.resets = np.zeros(host.E, np.int64)

    @property
    def state(self):
        return self.o.state

    def _rule(self):
        before = {k: self.o.state[k].copy() for k in ("shape", "nav", "need_reset")}
        ped_host.apply(self.o.state, self.o.k, self.ped)
        self.cover.note(before, self.o.state, self.host.E, self.host.cap)
        self.resets += before["need_reset"] != 0

    def reset(self):
        self.o.state["need_reset"][:] = 1      # BatchedEngine.reset: every env is about to be restored when md_ped runs
        self._rule()
        self.o.reset()

    def step(self, actions):
        self._rule()
        self.o.step(actions)


def _check(env, res, orc, where):
    st = env.engine.download_state()
    assert_state_equal(st, orc.state, keys=list(st), where=where)
    if res is not None:
        obs, reward, terminated, truncated, _ = res
        E = env.num_envs
        assert obs.cpu().numpy().tobytes() == orc.state["obs"].tobytes(), where
        assert reward.cpu().numpy().tobytes() == orc.state["reward"].tobytes(), where
        done = orc.state["done_out"].reshape(E, 4)
        assert np.array_equal(terminated.cpu().numpy().reshape(E), done[:, 0] != 0), where
        assert np.array_equal(truncated.cpu().numpy().reshape(E), done[:, 1] != 0), where


def _parity(seed, steps=STEPS, cover=True, env_cls=None, **extra):
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = (env_cls or BatchedMetaDriveEnv)(dict(PG, start_seed=seed, **extra))
    E = env.num_envs
    env.reset()
    orc = PedOracle(env.engine.host)
    orc.reset()
    _check(env, None, orc, "reset")
    for t in range(steps):
        a = scripted_actions(E, 1, t)
        res = env.step(a[:, 0])
        orc.step(a)
        _check(env, res, orc, "step %d" % t)
    assert (orc.resets >= 2).all(), orc.resets        # the reset of env.reset() and an auto-reset, in every env: none was skipped
    n = ped_host.driven_slots(orc.state, E, env.engine.cap).sum(axis=1)
    assert (n == env.config["num_pedestrians"]).all(), n
    if cover:
        assert orc.cover.kerb_holds >= 1 and orc.cover.mid_stops >= 1, (orc.cover.kerb_holds, orc.cover.mid_stops)
    return env, orc


def test_parity():
    seed, extra = PARITY_RUNS["default"]
    env, orc = _parity(seed, **extra)
    assert env.engine.host.step_kernel == "wg" and env.engine.k.traffic_mode == 0 and env.engine.cap <= 64
    pos, phase, slot = [x.cpu().numpy() for x in env.pedestrian_state()]
    assert pos.shape == (8, 3, 2) and phase.shape == slot.shape == (8, 3)
    want = np.nonzero(ped_host.driven_slots(orc.state, 8, env.engine.cap))[1].reshape(8, 3)
    assert np.array_equal(slot, want)
    sh = orc.state["shape"].reshape(8, -1)
    assert np.array_equal(pos[..., 0], np.take_along_axis(sh["cx"], want, 1)) and np.array_equal(pos[..., 1], np.take_along_axis(sh["cy"], want, 1))
    assert np.array_equal(phase, np.take_along_axis(orc.state["nav"]["toll_state"].reshape(8, -1), want, 1))


@pytest.mark.parametrize("name", ["respawn", "wave", "cap96", "envs5", "one"])
def test_parity_variants(name):
    seed, extra = PARITY_RUNS[name]
    env, _ = _parity(seed, **extra)
    eng = env.engine
    assert eng.host.step_kernel == extra.get("step_kernel", "wg")
    assert eng.cap == extra.get("mover_capacity", eng.cap) and eng.E == extra.get("num_envs", 8)
    assert eng.k.traffic_mode == (1 if "traffic_mode" in extra else 0)


@pytest.mark.parametrize("cls,extra", [
    ("BatchedSafeMetaDriveEnv", dict()),                                          # props above the pedestrians' slots
    ("BatchedVaryingDynamicsEnv", dict()),
    ("BatchedMetaDriveEnv", dict(traffic_mode="hybrid")),
    ("BatchedTopDownMetaDrive", dict(resolution_size=32)),
    ("BatchedTopDownMetaDriveEnvV2", dict(resolution_size=32)),
], ids=["safe", "varying", "hybrid", "topdown", "topdown_v2"])
def test_parity_other_classes_and_modes(cls, extra):
    """State parity over 40 steps and an auto-reset in the other classes and the traffic mode the feature is built for (the
    top-down image is those classes' own tests' business); the kerb hold and the mid-crossing stop are asserted by the parity runs
    above."""
    import metadrive_ped_amd.envs as envs
    env = getattr(envs, cls)(dict(PG, start_seed=19, **extra))
    env.reset()
    eng = env.engine
    orc = PedOracle(eng.host)
    orc.reset()
    for t in range(40):
        a = scripted_actions(8, 1, t)
        env.step(a[:, 0])
        orc.step(a)
        st = eng.download_state()
        assert_state_equal(st, orc.state, keys=list(st), where="%s step %d" % (cls, t))
    assert (orc.resets >= 2).all()
    assert (ped_host.driven_slots(orc.state, 8, eng.cap).sum(axis=1) == 3).all()
    if "resolution_size" in extra:
        assert tuple(env._obs().shape)[:3] == (8, 32, 32)


def test_parity_lane_change_agent():
    """agent_policy=LaneChangePolicy: the agents' PID rows hold the lane-change PIDs (tests/lane_change_host.py restates them); the
    pedestrians' PID rows hold their crossings -- the two never meet"""
    import lane_change_host as lh
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(PG, start_seed=19, agent_policy="LaneChangePolicy", discrete_action=True))
    env.reset()
    eng = env.engine
    lco = lh.LaneChangeOracle(eng.host)
    orc = PedOracle(eng.host, orc=lco.o)
    orc.reset()
    lco.pid = lco.o.state["pid"].copy()
    rng = np.random.RandomState(4)
    # what tests/test_gpu_lane_change.py compares (the oracle runs with agent_idm = 0), and the rows the pedestrians live in
    keys = ["shape", "dyn", "nav", "pid", "action", "flags", "obs", "reward", "cost", "step_info", "need_reset", "route_nodes",
            "route_roads", "final_lane", "idm_rand", "shape0", "dyn0", "nav0", "pid0"]
    for t in range(40):
        d = np.zeros((8, 1, 2), np.float32)
        d[..., 0] = rng.randint(-1, 2, (8, 1))
        d[..., 1] = rng.choice(np.float32([0.0, 0.5, 1.0]), (8, 1))
        eng.step(eng.torch.from_numpy(d).to(eng.device))
        orc._rule()
        lco.step(d)
        ref = {k: v.copy() for k, v in lco.o.state.items()}
        rows = lco.agent_rows()
        for k in lh.PID_ERRS:
            ref["pid"][k][rows] = lco.pid[k][rows]
        assert_state_equal(eng.download_state(), ref, keys=keys, where="lane change step %d" % t)
    assert (orc.resets >= 2).all()


def test_parity_idm_agent():
    """agent_policy=IDMPolicy: the agent drives itself (the RESPAWN variant carries that code), no actions"""
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(PG, start_seed=19, agent_policy="IDMPolicy", num_envs=4, num_scenarios=4))
    env.reset()
    orc = PedOracle(env.engine.host)
    orc.reset()
    for t in range(40):
        res = env.step(None)
        orc.step(None)
        _check(env, res, orc, "idm step %d" % t)
    assert (orc.resets >= 2).all()


def test_user_spawned_pedestrian_keeps_its_velocity():
    from metadrive_ped_amd import participants as P
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(PG, start_seed=19, mover_capacity=32, horizon=1000))
    env.reset()
    eng = env.engine
    orc = PedOracle(eng.host)
    orc.reset()
    at = eng.shape_f[:, 0, 0:2].cpu().numpy() + np.float32([12.0, 6.0])
    slot = env.spawn_object("pedestrian", at, heading_theta=0.5)
    env.set_velocity(slot, [1, 0], 1.4, in_local_frame=True)
    assert slot == P.spawn(orc.state, 8, 32, 1, "pedestrian", at, heading_theta=0.5)
    P.set_velocity(orc.state, 8, 32, slot, [1, 0], 1.4, in_local_frame=True)
    assert not ped_host.driven_slots(orc.state, 8, 32)[:, slot].any() and ped_host.driven_slots(orc.state, 8, 32).sum() == 24
    v0 = eng.dyn_f[:, slot, 1:4].cpu().numpy().copy()
    assert np.allclose(v0[:, 0], 1.4, atol=1e-5)
    for t in range(20):
        a = scripted_actions(8, 1, t)
        res = env.step(a[:, 0])
        orc.step(a)
        _check(env, res, orc, "participant step %d" % t)
        there = orc.resets == 1                   # a participant is gone when its env resets itself
        assert eng.dyn_f[:, slot, 1:4].cpu().numpy()[there].tobytes() == v0[there].tobytes()
    assert there.sum() >= 4
    moved = eng.shape_f[:, slot, 0:2].cpu().numpy() - at
    assert np.allclose(moved[there], 20 * 0.1 * v0[there, 1:3], atol=1e-3)
    assert orc.cover.phases >= {abi.PED_CROSS_AB, abi.PED_CROSS_BA} or orc.cover.kerb_holds > 0      # the policy walkers were at work


def _pg_env(steps=12, **kw):
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(PG, start_seed=19, **kw))
    env.reset()
    for t in range(steps):
        env.step(scripted_actions(env.num_envs, 1, t)[:, 0])
    return env


def test_snapshot_and_restore_reproduce_the_run():
    env = _pg_env()
    snap = env.snapshot()

    def run():
        out = []
        for t in range(12, 37):
            res = env.step(scripted_actions(8, 1, t)[:, 0])
            out.append(([x.cpu().numpy().copy() for x in res[:4]], env.engine.download_state()))
        return out

    first = run()
    assert any(st["need_reset"].any() for _, st in first), "the run must pass an auto-reset"
    env.restore(snap)
    again = run()
    for t, ((oa, sa), (ob_, sb)) in enumerate(zip(first, again)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(oa, ob_)), t
        assert_state_equal(sa, sb, keys=list(sa), where="after restore, step %d" % t)
    walked = first[-1][1]["shape"].view(np.uint8).reshape(8, -1) != first[0][1]["shape"].view(np.uint8).reshape(8, -1)
    assert walked.any()


def test_branch_to_an_env_on_another_map_matches_the_oracle():
    import oracle_binding as ob
    from metadrive_ped_amd import branch
    env = _pg_env()
    eng = env.engine
    before = eng.download_state()
    env_map = eng.world_dev["env_map"].view(eng.torch.int32).cpu().numpy().copy()
    assert len(set(env_map.tolist())) == 8
    pairs = [(3, 0), (3, 6), (5, 1)]
    env.branch([3, 3, 5], [0, 6, 1])
    branch.apply_host(before, env_map, pairs)
    assert_state_equal(eng.download_state(), before, keys=list(before), where="after branch")
    o = ob.OracleWorld(eng.host, state=before)
    o._env_map = np.ascontiguousarray(env_map, np.int32)
    o.w.env_map = o._env_map.ctypes.data
    orc = PedOracle(eng.host, orc=o)
    for t in range(12, 52):
        a = scripted_actions(8, 1, t)
        a[0], a[6], a[1] = a[3], a[3], a[5]
        res = env.step(a[:, 0])
        orc.step(a)
        _check(env, res, orc, "branched, step %d" % t)
        st = orc.state["shape"].view(np.uint8).reshape(8, -1)
        assert np.array_equal(st[0], st[3]) and np.array_equal(st[6], st[3]) and np.array_equal(st[1], st[5])
    assert (orc.resets >= 1).all()


def test_pg_walk_carries_the_pedestrians():
    import pg_walk_host as ph
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    cfg = make_config(dict(walk_scenarios=True, num_envs=6, num_scenarios=10, map=2, traffic_density=0.15, horizon=20, start_seed=30,
                           num_pedestrians=2))
    eng = BatchedEngine(cfg)
    o = ph.PgWalkOracle(eng.host)
    orc = PedOracle(eng.host, orc=o)
    eng.reset()
    o.state["need_reset"][:] = 1
    orc._rule()
    o.reset()
    keys = list(eng.download_state())
    assert_state_equal(eng.download_state(), o.state, keys=keys, where="walk reset")
    for t in range(2 * 21 + 2):
        a = scripted_actions(6, 1, t, seed=3)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        assert_state_equal(eng.download_state(), o.state, keys=keys, where="walk step %d" % t)
        assert np.array_equal(eng.world_dev["env_map"].view(torch.int32).cpu().numpy(), o.env_map), t
    st = eng.download_state()
    assert (st["walk_ep"] >= 2).all()
    # the walkers of the scene an env plays now are that scene's
    n = ped_host.driven_slots(st, 6, eng.cap).sum(axis=1)
    assert n.tolist() == [len(eng.host.scenes[eng.host.seeds[int(p)]].ped_slots) for p in st["scene_of"]]


def test_random_traffic_carries_the_pedestrians():
    import oracle_binding as ob
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    E, K = 6, 3
    cfg = make_config(dict(num_envs=E, num_scenarios=3, map=3, traffic_density=0.2, start_seed=40, random_traffic=True, traffic_draws=K,
                           horizon=20, num_pedestrians=2))
    eng = BatchedEngine(cfg)
    hosts = eng.draw_hosts_
    assert len(hosts) == K
    orc = PedOracle(eng.host)
    eng.reset()
    orc.reset()
    cap, idx = eng.cap, np.zeros(E, np.int64)
    twins = dict(param="param0", route_nodes="route_nodes0", route_roads="route_roads0", final_lane="final_lane0")
    for t in range(2 * 21 + 2):
        a = scripted_actions(E, 1, t)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        for e in np.nonzero(orc.state["need_reset"])[0]:            # what md_swap_draw does
            idx[e] = (idx[e] + 1) % K
            rows = slice(e * cap, (e + 1) * cap)
            for k in BatchedEngine.DRAW_ARRAYS:
                if k in orc.state:
                    orc.state[k][rows] = hosts[idx[e]].state[k][rows]
                    if k in twins and twins[k] in orc.state:
                        orc.state[twins[k]][rows] = hosts[idx[e]].state[k][rows]
        st = eng.download_state()
        assert_state_equal(st, orc.state, keys=list(st), where="random_traffic step %d" % t)
    assert (idx > 0).all() and (ped_host.driven_slots(orc.state, E, cap).sum(axis=1) == 2).all()


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("md_") or name == "md_last_error":
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


def test_one_more_launch_per_step():
    calls = {}
    for n in (0, 3):
        env = _pg_env(steps=2, num_pedestrians=n)
        lib = env.engine.lib = _CountingLib(env.engine.lib)
        env.step(scripted_actions(8, 1, 2)[:, 0])
        calls[n] = list(lib.calls)
    assert "md_ped" not in calls[0] and calls[0].count("md_step") == 1
    assert calls[3] == ["md_ped"] + calls[0]
