"""The vector scene observation of scenario mode on the MI355X (md_scenario_vector_obs, include/md_scenario_vector_obs.h):
env.vector_obs() and the engine-owned history bit for bit against the gcc host build of the header (tests/scenario_vector_obs_host.py),
run on the state downloaded after every step; replayed and reactive traffic, the smallest shapes, the defaults and the ceilings; the
walk; the env surface; one launch per step and none without the key."""
import numpy as np
import pytest

import scenario_vector_obs_host as sh
from metadrive_ped_amd import abi
from metadrive_ped_amd.scenario import synthetic_scenarios

pytestmark = pytest.mark.gpu

_POOLS = {}


def _pool(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _POOLS:
        _POOLS[key] = synthetic_scenarios(n, 900, T=80, **kw)
    return _POOLS[key]


def _env(scenarios, vo, **kw):
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    cfg = dict(num_envs=len(scenarios), num_scenarios=len(scenarios), horizon=400, scenario_vector_obs=vo)
    cfg.update(kw)
    return BatchedScenarioEnv(cfg, scenarios=scenarios)


def _follow(obs, n_side=12):
    """a small route follower on the navigation dims (lateral, heading error), [E, 2]"""
    o_navi = (n_side or 2) + 6 + 1
    a = np.zeros((len(obs), 2), np.float32)
    a[:, 0] = np.clip(6.0 * (obs[:, o_navi + 19] - 0.5) + 2.0 * (obs[:, o_navi + 18] - 0.5), -1, 1)
    a[:, 1] = 0.3
    return a


class Parity:
    """The host build stepped beside the device: its own history rows, fed the state the device's launch read"""
    def __init__(self, env):
        self.env, self.eng = env, env.engine
        h = self.eng.host
        self.hv = sh.HostScenarioVectorObs(env.config["scenario_vector_obs"], h.E, h.cap, h.map_pieces)
        self.scene_of = None     # a walking batch: every env's scene as it was before the step's swap moved the ended envs on

    def check(self, where):
        state = self.eng.download_state()
        seen = dict(state)
        if "scene_of" in state:
            if self.scene_of is not None:
                seen["scene_of"] = self.scene_of
            self.scene_of = state["scene_of"].copy()
        w, s, k, keep = sh.structs_of(self.eng.host, seen)
        self.hv.run(w, s, k)
        dev, want = {n: t.cpu().numpy() for n, t in self.env.vector_obs().items()}, self.hv.outputs()
        assert list(dev) == list(sh.OUTPUTS)
        for name in sh.OUTPUTS:
            assert dev[name].shape == want[name].shape and dev[name].dtype == want[name].dtype, (where, name)
            if dev[name].tobytes() != want[name].tobytes():
                bad = np.argwhere(dev[name] != want[name])[:4]
                raise AssertionError("%s: %s differs at %s: device %s, host %s" % (where, name, bad.tolist(), [dev[name][tuple(i)] for i in bad],
                                                                                 [want[name][tuple(i)] for i in bad]))
        hist, want_hist = self.eng.vector_obs_history(), self.hv.history()
        for name in sh.HISTORY:
            assert hist[name].tobytes() == want_hist[name].tobytes(), (where, name)
        return dev, state


def _run(env, steps):
    """reset, then `steps` steps of the follower with the parity check after each; -> (Parity, the outputs of every check)"""
    obs, _ = env.reset()
    p = Parity(env)
    outs = [p.check("reset")[0]]
    for t in range(steps):
        obs = env.step(_follow(obs.cpu().numpy()))[0]
        outs.append(p.check("step %d" % t)[0])
    return p, outs


# -- 1. bit-exact against the host build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reactive", [True, False])
def test_bit_exact_against_the_host_build(reactive):
    env = _env(_pool(4), dict(sh.SMALL), reactive_traffic=reactive)
    p, outs = _run(env, 30)
    pieces = env.engine.host.map_pieces
    assert (np.diff(pieces["map_off"]) > 700).all(), "the strided loop over the pieces runs past 64"
    me = env.engine.download_state()["shape"].reshape(4, -1)[:, 0]
    for e in range(4):      # ... and so does the compaction: over 200 candidates inside the radius
        a, b = pieces["map_off"][e], pieces["map_off"][e + 1]
        d2 = ((pieces["map_xy"][a:b, :, 0] - me["cx"][e]) ** 2 + (pieces["map_xy"][a:b, :, 1] - me["cy"][e]) ** 2).min(1)
        assert (d2 <= 2500.0).sum() > 200
    assert outs[0]["ego_mask"].tolist() == [[1, 0, 0]] * 4 and (p.hv.history()["cursor"][:, 1] == 3).all()
    last = outs[-1]
    assert last["ego_mask"].all() and last["route_mask"].any() and last["map_mask"][:, :, 0].all() and last["agents_mask"][:, 0, 0].all()
    kinds = np.concatenate([o["agents_meta"][..., 3].ravel() for o in outs])
    assert (kinds == abi.KIND_VEHICLE).any()


def test_default_shapes():
    env = _env(_pool(4), {})
    p, outs = _run(env, 8)
    spec = env.vector_obs_spec()
    assert outs[-1]["map"].shape == (4, 32, 8, 2) and outs[-1]["agents"].shape == (4, 8, 5, 4)
    assert outs[-1]["map_mask"][:, :, 0].all() and outs[-1]["route_mask"][:, :8].all() and outs[-1]["ego_mask"].all()
    assert {k: (tuple(v.shape), v.dtype.type) for k, v in outs[-1].items()} == spec
    assert len(np.unique(outs[-1]["map_meta"][..., 0])) == 3, "lanes, lines and edges are all near the road"


# -- 2. the ceilings, and more than 64 slots: two slots per lane -------------------------------------------------------------------------
def test_ceilings():
    env = _env(_pool(2, n_vehicles=60), dict(sh.CEILINGS))
    obs, _ = env.reset()
    assert env.engine.cap == 72
    p = Parity(env)
    p.check("reset")
    for t in range(9):
        obs = env.step(_follow(obs.cpu().numpy()))[0]
        dev, state = p.check("step %d" % t)
    assert dev["agents_mask"][:, :, 0].all(), "sixteen neighbours within 50 m"
    assert dev["ego_mask"].all() and dev["agents_mask"][:, :, 7].any(), "eight frames held"
    flags = state["shape"]["flags"].reshape(2, 72)
    assert ((flags[:, 64:] & abi.F_ALIVE) != 0).any()


# -- 3. the walk: the step that ends an episode is observed on the scene it belongs to ------------------------------------------------
def test_a_walking_env_s_last_frame_is_read_on_its_own_scene():
    env = _env(_pool(9), dict(sh.SMALL), num_envs=6, walk_scenarios=True, sequential_seed=True, horizon=8)
    obs, _ = env.reset()
    p = Parity(env)
    dev, state = p.check("reset")
    assert dev["ego_mask"].tolist() == [[1, 0, 0]] * 6
    moved, resets = 0, 0
    for t in range(3 * 9 + 2):
        before = p.scene_of.copy()
        obs, r, term, trunc, _ = env.step(_follow(obs.cpu().numpy()))
        dev, state = p.check("step %d" % t)          # the host build runs on the scenes as they were before the swap
        moved += int((state["scene_of"] != before).sum())
        fresh = state["nav"]["steps"].reshape(6, -1)[:, 0] == 0
        resets += int(fresh.sum())
        assert dev["ego_mask"][fresh].tolist() == [[1, 0, 0]] * int(fresh.sum()), t
    assert moved >= 6 and resets >= 18, "every env passes three episode ends inside the run (envs 3 .. 5 of 6 workers over 9 scenes replay theirs)"


# -- 4. the env surface ------------------------------------------------------------------------------------------------------------------
def test_env_surface_and_the_replayed_ego():
    env = _env(_pool(4), dict(sh.SMALL), agent_policy="ReplayEgoCarPolicy")
    env.reset()
    p = Parity(env)
    p.check("reset")
    for t in range(6):
        env.step(None)
        dev, _ = p.check("step %d" % t)
    out, spec = env.vector_obs(), env.vector_obs_spec()
    assert list(out) == list(spec) == list(abi.SCENARIO_VECTOR_OBS_OUTPUTS)
    for name, t in out.items():
        assert t.device.type == "cuda" and tuple(t.shape) == spec[name][0] and t.cpu().numpy().dtype.type == spec[name][1], name
        assert t.data_ptr() >= env.engine.vector_obs_rows.data_ptr(), "a view of the engine's rows"
    # the replayed ego sits on its own recorded trajectory: the waypoints lie straight ahead of it
    assert dev["route_mask"].all() and (np.abs(dev["route"][:, 0, 1]) < 0.5).all() and (dev["route"][:, 0, 0] > 3.5).all()
    st = env.get_state()
    env.set_state(st)
    assert not env.engine.vector_obs_history()["cursor"].any(), "set_state forgets the history"
    env.step(None)
    assert env.vector_obs()["ego_mask"].cpu().numpy().tolist() == [[1, 0, 0]] * 4


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("md_") or name == "md_last_error":
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_one_launch_per_step_and_none_without_the_key():
    counts = {}
    for key, vo in (("on", dict(sh.SMALL)), ("off", None)):
        env = _env(_pool(4), vo)
        obs, _ = env.reset()
        lib = env.engine.lib = _CountingLib(env.engine.lib)
        for t in range(5):
            obs = env.step(_follow(obs.cpu().numpy()))[0]
        counts[key] = dict(lib.calls)
        if vo is None:
            e = env.engine
            assert e.vector_obs_rows is None and e.vector_obs_hist is None and e.scenario_map_dev is None and e._svo is None
            assert e.host.map_pieces is None
            with pytest.raises(RuntimeError, match="scenario_vector_obs"):
                env.vector_obs()
    assert counts["on"].pop("md_scenario_vector_obs") == 5
    assert counts["on"] == counts["off"] and "md_scenario_vector_obs" not in counts["off"] and "md_vector_obs" not in counts["off"]
