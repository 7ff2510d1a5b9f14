"""The closed-loop driving metrics of scenario mode on the MI355X (md_scenario_metrics, include/md_scenario_metrics.h):
env.scenario_metrics() bit for bit against the gcc host build of the header (tests/scenario_metrics_host.py), run on the state
downloaded after every step -- replayed and reactive traffic, a driven and a replayed ego, episodes that end, reset inside md_step and
latch, with lights and without, the sweep's ceiling --; the replayed ego's divergence and finite differences against the answer worked
out from the description and the downloaded dyn rows alone; the walk; one launch per step and none without the key."""
import numpy as np
import pytest

import scenario_metrics_host as mh
from metadrive_ped_amd import abi
from metadrive_ped_amd.scenario import synthetic_scenarios

pytestmark = pytest.mark.gpu

T = 80
NAMES = mh.OUTPUTS + ("episode", "history")
_POOLS = {}


def _pool(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _POOLS:
        _POOLS[key] = synthetic_scenarios(n, 900, T=T, **kw)
    return _POOLS[key]


def _env(scenarios, sm, **kw):
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    cfg = dict(num_envs=len(scenarios), num_scenarios=len(scenarios), horizon=400, scenario_metrics=sm)
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
    """The host build beside the device, fed the state (and the agent_light) the device's launch read; both keep their own history
    and accumulators from the reset on"""
    def __init__(self, env):
        self.env, self.eng = env, env.engine
        self.lights = env.config["traffic_lights"] is not None
        self.hm = mh.HostScenarioMetrics(env.config["scenario_metrics"], self.eng.host.E, lights=self.lights)
        self.scene_of = None     # a walking batch: every env's scene as it was before the step's swap moved the ended envs on

    def check(self, where):
        state = self.eng.download_state()
        seen = dict(state)
        if "scene_of" in state:
            if self.scene_of is not None:
                seen["scene_of"] = self.scene_of
            self.scene_of = state["scene_of"].copy()
        if self.lights:
            self.hm.agent_light[:] = self.env.traffic_lights()["agent_light"].cpu().numpy()
        w, s, k, keep = mh.structs_of(self.eng.host, seen)
        self.hm.run(w, s, k)
        dev, want = {n: t.cpu().numpy() for n, t in self.env.scenario_metrics().items()}, self.hm.outputs()
        assert sorted(dev) == sorted(NAMES)
        for name in NAMES:
            assert dev[name].shape == want[name].shape and dev[name].dtype == want[name].dtype, (where, name)
            if dev[name].tobytes() != want[name].tobytes():
                bad = np.argwhere(dev[name].view(np.int32) != want[name].view(np.int32))[:4]
                raise AssertionError("%s: %s differs at %s: device %s, host %s" % (where, name, bad.tolist(), [dev[name][tuple(i)] for i in bad],
                                                                                 [want[name][tuple(i)] for i in bad]))
        return dev, state


# -- 1. bit-exact against the host build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reactive,replay,horizon,lights", [(True, False, 5, True), (False, True, 400, False), (True, True, 400, True),
                                                            (False, False, 5, False)])
def test_bit_exact_against_the_host_build(reactive, replay, horizon, lights):
    scenes = _pool(5, n_lights=3) if lights else _pool(5)
    env = _env(scenes, {}, reactive_traffic=reactive, horizon=horizon, traffic_lights={} if lights else None,
               **(dict(agent_policy="ReplayEgoCarPolicy") if replay else {}))
    obs, _ = env.reset()
    p = Parity(env)
    dev, _ = p.check("reset")
    assert not dev["episodes"].any() and not dev["last_episode"].any() and not dev["episode"][:, mh.EPISODE("steps")].any()
    observer = (1 << mh.STEP("speed")) | (1 << mh.STEP("ttc")) | ((1 << mh.STEP("on_red")) if lights else 0)
    assert ((dev["step_valid"] & observer) == observer).all() and not (dev["step_valid"] & (0x1F8 if lights else 0x5F8)).any()
    jerked = hit = 0
    for t in range(13):
        obs, _, term, trunc, info = env.step(None if replay else _follow(obs.cpu().numpy()))
        dev, _ = p.check("step %d" % t)
        jerked += int(((dev["step_valid"] >> mh.STEP("jerk")) & 1).sum())
        hit += int((dev["ttc_slot"] >= 0).sum())
        assert info["log_divergence"].cpu().numpy().tobytes() == dev["step"][:, mh.STEP("log_divergence")].tobytes()
        assert info["time_to_collision"].cpu().numpy().tobytes() == dev["step"][:, mh.STEP("ttc")].tobytes()
        assert info["comfortable"].cpu().numpy().tolist() == (dev["episode"][:, mh.EPISODE("comfort_violation_steps")] == 0).tolist()
    assert jerked > 0, "the second differences were reached"
    if horizon == 5:     # steps 1 .. 5, the reset inside md_step, 1 .. 5 again, the reset, one more
        assert dev["episodes"].tolist() == [2] * 5 and (dev["last_episode"][:, mh.EPISODE("steps")] == 5).all()
        assert (dev["episode"][:, mh.EPISODE("steps")] == 1).all()
    else:
        assert not dev["episodes"].any() and (dev["episode"][:, mh.EPISODE("steps")] == 13).all()


# -- 2. known answer from the description and the dyn rows alone -----------------------------------------------------------------------
def test_the_replayed_ego_never_strays_and_its_rates_are_the_dyn_rows_differences():
    env = _env(_pool(3), {}, agent_policy="ReplayEgoCarPolicy")
    env.reset()
    h = env.engine.host
    D = mh.step_period()
    prev = env.engine.download_state()["dyn"].reshape(h.E, h.cap)[:, 0].copy()
    valid_bits = (1 << mh.STEP("log_divergence")) | (1 << mh.STEP("log_heading_error"))
    moved = strayed = 0
    for k in range(1, 13):
        env.step(None)
        m = {n: t.cpu().numpy() for n, t in env.scenario_metrics().items()}
        dyn = env.engine.download_state()["dyn"].reshape(h.E, h.cap)[:, 0].copy()
        for e in range(h.E):
            fl = int(h.tracks["shape"][k, e * h.cap]["flags"])      # after step k the replayed ego stands on frame k of its track
            exists = k < T and bool(fl & abi.F_ALIVE) and (fl & abi.KIND_MASK) != abi.KIND_NONE
            assert (int(m["step_valid"][e]) & valid_bits) == (valid_bits if exists else 0), (k, e)
            assert m["step"][e, 0] == 0.0 and m["step"][e, 1] == 0.0, (k, e)
            strayed += int(exists)
            want = (np.float32(dyn[e]["speed"]), ) + mh.rates_f32(dyn[e]["speed"], dyn[e]["heading"], prev[e]["speed"], prev[e]["heading"], D)
            assert np.asarray(want, np.float32).tobytes() == m["step"][e, 2:6].tobytes(), (k, e, want, m["step"][e, 2:6])
            moved += int(m["step"][e, mh.STEP("lon_accel")] != 0.0)
        prev = dyn
    assert strayed > 0 and moved > 0, "the case cannot pass empty: valid SDC frames, and a recorded drive that changes its speed"


# -- 3. the walk -------------------------------------------------------------------------------------------------------------------------
def test_a_walking_env_s_last_frame_is_scored_on_its_own_scene():
    env = _env(_pool(4), {}, num_envs=3, walk_scenarios=True, sequential_seed=True, horizon=5)
    obs, _ = env.reset()
    p = Parity(env)
    dev, state = p.check("reset")
    episodes, moved = np.zeros(3, np.int64), 0
    for t in range(13):
        before = p.scene_of.copy().reshape(-1)
        obs, _, term, trunc, info = env.step(_follow(obs.cpu().numpy()))
        dev, state = p.check("step %d" % t)          # the host build runs on the scenes as they were before the swap
        ended = (term | trunc).cpu().numpy().astype(bool)
        episodes += ended
        assert dev["episodes"].tolist() == episodes.tolist(), t
        rc = info["route_completion"].cpu().numpy()
        assert dev["last_episode"][ended, mh.EPISODE("route_completion")].tobytes() == rc[ended].tobytes()
        # the ending step's divergence is measured against the OLD scene's SDC track, frame 5
        for e in np.nonzero(ended)[0]:
            h = env.engine.host
            fr = h.tracks["shape"][5, before[e] * h.cap]
            me = state["shape"].reshape(3, h.cap)[e, 0]
            assert int(fr["flags"]) & abi.F_ALIVE
            dx, dy = np.float32(me["cx"]) - np.float32(fr["cx"]), np.float32(me["cy"]) - np.float32(fr["cy"])
            want = np.sqrt(np.float32(dx * dx) + np.float32(dy * dy), dtype=np.float32)
            assert dev["step"][e, 0] == want and dev["last_episode"][e, mh.EPISODE("fde")] == want, (t, e)
            moved += int(before[e] != np.asarray(state["scene_of"]).reshape(-1)[e])
    assert episodes.tolist() == [2, 2, 2] and moved >= 2, "the envs ended episodes and moved on to other scenes"


# -- 4. the sweep's ceiling --------------------------------------------------------------------------------------------------------------
def test_the_ceiling_of_the_sweep():
    env = _env(_pool(5), dict(ttc_samples=abi.MD_SM_MAX_TTC_SAMPLES, ttc_dt=0.25), reactive_traffic=True)
    obs, _ = env.reset()
    p = Parity(env)
    p.check("reset")
    found = 0
    for t in range(6):
        obs = env.step(_follow(obs.cpu().numpy()))[0]
        dev, state = p.check("step %d" % t)
        found += int((dev["ttc_slot"] >= 0).sum())
    present = (state["shape"]["flags"].reshape(5, -1)[:, 1:] & abi.F_ALIVE) != 0
    assert present.sum(1).min() >= 1, "every scene has movers for the sweep to test"
    assert (dev["step"][dev["ttc_slot"] < 0, mh.STEP("ttc")] == np.float32(64) * np.float32(0.25) + np.float32(0.25)).all()


# -- 5. the launch count, and nothing else changes ---------------------------------------------------------------------------------------
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


def test_one_launch_per_step_none_without_the_key_and_the_same_step_outputs():
    counts, outs = {}, {}
    scenes = _pool(4)
    for key, sm in (("on", {}), ("off", None)):
        env = _env(scenes, sm, reactive_traffic=True)
        obs, info = env.reset()
        lib = env.engine.lib = _CountingLib(env.engine.lib)
        rows = [obs.cpu().numpy().copy()]
        for t in range(6):
            obs, r, term, trunc, info = env.step(_follow(obs.cpu().numpy()))
            rows += [x.cpu().numpy().copy() for x in (obs, r, info["cost"], term, trunc, env.engine.flags)]
            for name in ("log_divergence", "time_to_collision", "comfortable"):
                assert (name in info) == (sm is not None)
        counts[key], outs[key] = dict(lib.calls), rows
        if sm is None:
            e = env.engine
            assert e._sm is None and e.scenario_metrics_rows is None and e.scenario_metrics_state is None and e.scenario_metrics_out is None
            for call in (env.scenario_metrics, env.scenario_metrics_spec):
                with pytest.raises(RuntimeError, match="scenario_metrics"):
                    call()
        else:
            spec = env.scenario_metrics_spec()
            for name, t_ in env.scenario_metrics().items():
                assert t_.device.type == "cuda" and tuple(t_.shape) == spec[name][0] and t_.cpu().numpy().dtype.type == spec[name][1], name
            env.reset()
            assert not env.scenario_metrics()["last_episode"].any() and not env.scenario_metrics()["episodes"].any()
    assert counts["on"].pop("md_scenario_metrics") == 6
    assert counts["on"] == counts["off"] and "md_scenario_metrics" not in counts["off"]
    assert len(outs["on"]) == len(outs["off"])
    for a, b in zip(outs["on"], outs["off"]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
