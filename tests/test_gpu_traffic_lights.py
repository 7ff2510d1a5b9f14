"""The traffic lights of scenario mode on the MI355X (md_traffic_lights, include/md_traffic_lights.h): env.traffic_lights() bit for
bit against the gcc host build of the header (tests/traffic_lights_host.py), run on the state downloaded after every step -- scenes
with 0, 1, 3 and 65 lights, status arrays shorter than the episode, replayed and reactive traffic, the ceilings --; the red-light flag
of a replayed ego against the answer worked out from the description alone; the walk; one launch per step and none without the key."""
import copy
import ctypes as C

import numpy as np
import pytest

import traffic_lights_host as th
from metadrive_ped_amd import abi
from metadrive_ped_amd.scenario import synthetic_scenarios

pytestmark = pytest.mark.gpu

T = 80
STATES = ["LANE_STATE_STOP", "LANE_STATE_GO", "LANE_STATE_CAUTION", None, "LANE_STATE_ARROW_STOP", "LANE_STATE_UNKNOWN",
          "LANE_STATE_FLASHING_CAUTION", "LANE_STATE_ARROW_GO", "LANE_STATE_FLASHING_STOP"]
_POOLS = {}


def _pool(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _POOLS:
        _POOLS[key] = synthetic_scenarios(n, 900, T=T, **kw)
    return _POOLS[key]


def with_lights(scenario, total, frames=None):
    """a copy of a synthetic description with lights added by hand up to `total`: light i on a lane feature of its own (a copy of
    lane i % 3), its stop point on or beside the ego's recorded path, i % 9 + 4 status frames (or `frames`) from a rotating list"""
    out = copy.deepcopy(scenario)
    feats, lights = out["map_features"], out["dynamic_map_states"]
    path = out["tracks"]["0"]["state"]["position"]
    for i in range(len(lights), total):
        key = "extra%d" % i
        feats[key] = copy.deepcopy(feats["lane%d" % (i % 3)])
        x, y = path[2 + (i * 7) % (T - 2), :2]
        side = ((i // 9) % 5 - 2) * 9.0             # every ninth light on the path, the others up to 18 m beside it
        n = frames or (i % 9 + 4)
        lights[key] = {"type": "TRAFFIC_LIGHT", "lane": key, "stop_point": np.asarray([x + side, y - 0.5 * side, 0.0], np.float32),
                       "state": {"object_state": [STATES[(i + f // 2) % len(STATES)] for f in range(n)]}, "metadata": {}}
    return out


def _env(scenarios, tl, **kw):
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    cfg = dict(num_envs=len(scenarios), num_scenarios=len(scenarios), horizon=400, traffic_lights=tl)
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
    """The host build beside the device, fed the state the device's launch read"""
    def __init__(self, env):
        self.env, self.eng = env, env.engine
        h = self.eng.host
        self.hv = th.HostTrafficLights(env.config["traffic_lights"], h.E, h.traffic_lights)
        self.scene_of = None     # a walking batch: every env's scene as it was before the step's swap moved the ended envs on

    def check(self, where):
        state = self.eng.download_state()
        seen = dict(state)
        if "scene_of" in state:
            if self.scene_of is not None:
                seen["scene_of"] = self.scene_of
            self.scene_of = state["scene_of"].copy()
        w, s, k, keep = th.structs_of(self.eng.host, seen)
        self.hv.run(w, s, k)
        dev, want = {n: t.cpu().numpy() for n, t in self.env.traffic_lights().items()}, self.hv.outputs()
        assert list(dev) == list(th.OUTPUTS)
        for name in th.OUTPUTS:
            assert dev[name].shape == want[name].shape and dev[name].dtype == want[name].dtype, (where, name)
            if dev[name].tobytes() != want[name].tobytes():
                bad = np.argwhere(dev[name] != want[name])[:4]
                raise AssertionError("%s: %s differs at %s: device %s, host %s" % (where, name, bad.tolist(), [dev[name][tuple(i)] for i in bad],
                                                                                 [want[name][tuple(i)] for i in bad]))
        return dev, state


# -- 1. bit-exact against the host build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reactive", [True, False])
def test_bit_exact_against_the_host_build(reactive):
    base = _pool(5)
    scenes = [base[0], with_lights(base[1], 1), _pool(5, n_lights=3)[2], with_lights(_pool(5, n_lights=3)[3], 65), with_lights(base[4], 3, frames=5)]
    env = _env(scenes, dict(num_lights=3, radius=80.0), reactive_traffic=reactive, agent_policy="ReplayEgoCarPolicy")
    env.reset()
    tables = env.engine.host.traffic_lights
    assert np.diff(tables["tl_off"]).tolist() == [0, 1, 3, 65, 3] and tables["max_scene_lights"] == 65
    assert (tables["tl_info"][:, 1] < 12).sum() > 50, "status arrays shorter than the episode"
    p = Parity(env)
    dev, _ = p.check("reset")
    assert not dev["agent_light"].any(), "no flag at the reset"
    assert dev["lights_mask"].sum(1).tolist() == [0, 1, 3, 3, 3]
    seen = np.zeros(5, np.uint8)
    for t in range(12):
        _, _, _, _, info = env.step(None)
        dev, _ = p.check("step %d" % t)
        seen |= dev["agent_light"]
        for name, bit in (("green_light", 1), ("yellow_light", 2), ("red_light", 4)):
            assert info[name].cpu().numpy().tolist() == ((dev["agent_light"] & bit) != 0).tolist()
    assert seen[0] == 0 and seen[3] == 7, "the ego of the 65-light scene drives through walls of every colour"


# -- 2. the ceilings ------------------------------------------------------------------------------------------------------------------
def test_ceilings():
    base = _pool(2)
    env = _env([with_lights(base[0], 1024), with_lights(base[1], 40)], dict(num_lights=32, radius=80.0), agent_policy="ReplayEgoCarPolicy")
    env.reset()
    assert env.engine.host.traffic_lights["max_scene_lights"] == abi.MD_TL_MAX_SCENE_LIGHTS == 1024
    p = Parity(env)
    dev, _ = p.check("reset")
    assert dev["lights_mask"].all() and dev["lights"].shape == (2, 32, 6)
    env.step(None)
    dev, _ = p.check("step 0")
    assert (np.diff(dev["lights"][:, :, 5], axis=1) >= 0).all(), "ascending in d2"


# -- 3. known answer end to end --------------------------------------------------------------------------------------------------------
def one_scene_tables(host, scene):
    """the tables of the scene alone, from the host scene's"""
    from metadrive_ped_amd.scenario import traffic_light_tables
    t = host.traffic_lights
    a, b = int(t["tl_off"][scene]), int(t["tl_off"][scene + 1])
    return traffic_light_tables([(t["tl_box"][a:b], [t["tl_status"][o:o + n] for o, n in t["tl_info"][a:b, :2]], t["ids"][scene])])


def test_the_replayed_ego_runs_the_reds_the_description_says():
    scenes = synthetic_scenarios(2, 900, T=T, n_lights=3)
    env = _env(scenes, {}, agent_policy="ReplayEgoCarPolicy")
    env.reset()
    h = env.engine.host
    steps = 70
    # the answer from the description alone: after step k the replayed ego stands on frame k of its track
    want = np.zeros((steps, 2), bool)
    for e in range(2):
        tables = one_scene_tables(h, e)
        for k in range(1, steps + 1):
            w, s, kk, st = th.light_world()
            st["shape"][0] = h.tracks["shape"][k, e * h.cap]
            st["nav"][0]["steps"] = k
            want[k - 1, e] = bool(int(th.HostTrafficLights({}, 1, tables).run(w, s, kk).out("agent_light")[0]) & abi.TL_BIT_RED)
    got = np.zeros((steps, 2), bool)
    for k in range(steps):
        got[k] = env.step(None)[4]["red_light"].cpu().numpy()
    assert want.any(), "the case cannot pass empty: the ego crosses a stop line on red"
    assert got.any() and got.tolist() == want.tolist()


# -- 4. the walk -------------------------------------------------------------------------------------------------------------------------
def test_a_walking_env_s_last_frame_is_read_on_its_own_scene():
    base = _pool(4)
    scenes = [base[0], with_lights(base[1], 3), with_lights(base[2], 1), with_lights(base[3], 2)]
    env = _env(scenes, dict(num_lights=3), num_envs=3, walk_scenarios=True, sequential_seed=True, horizon=5)
    obs, _ = env.reset()
    counts = np.diff(env.engine.host.traffic_lights["tl_off"])
    assert counts.tolist() == [0, 3, 1, 2]
    p = Parity(env)
    dev, state = p.check("reset")
    assert dev["lights_mask"].sum(1).tolist() == [0, 3, 1]
    moved = 0
    for t in range(13):
        before = p.scene_of.copy()
        obs = env.step(_follow(obs.cpu().numpy()))[0]
        dev, state = p.check("step %d" % t)          # the host build runs on the scenes as they were before the swap
        now = state["scene_of"].reshape(-1)
        ended = now != before.reshape(-1)
        moved += int(ended.sum())
        # the frame at the episode's end shows the OLD scene's lights; the step after, the new scene's (all within the radius)
        assert dev["lights_mask"].sum(1).tolist() == np.minimum(counts[before.reshape(-1)], 3).tolist(), t
    assert moved >= 2, "env 0 alternates between a scene without lights and one with two"


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
    scenes = _pool(4, n_lights=3)
    for key, tl in (("on", dict(num_lights=3)), ("off", None)):
        env = _env(scenes, tl, reactive_traffic=True)
        obs, info = env.reset()
        lib = env.engine.lib = _CountingLib(env.engine.lib)
        rows = [obs.cpu().numpy().copy()]
        for t in range(6):
            obs, r, term, trunc, info = env.step(_follow(obs.cpu().numpy()))
            rows += [x.cpu().numpy().copy() for x in (obs, r, info["cost"], term, trunc, env.engine.flags)]
            assert ("red_light" in info) == (tl is not None) and ("green_light" in info) == (tl is not None)
        counts[key], outs[key] = dict(lib.calls), rows
        if tl is None:
            e = env.engine
            assert e._tl is None and e.traffic_lights_rows is None and e.traffic_lights_dev is None and e.traffic_lights_out is None
            assert e.host.traffic_lights is None
            with pytest.raises(RuntimeError, match="traffic_lights"):
                env.traffic_lights()
        else:
            assert env.traffic_light_ids(1) == ["lane0", "lane1", "lane2"]
            spec = env.traffic_lights_spec()
            for name, t_ in env.traffic_lights().items():
                assert t_.device.type == "cuda" and tuple(t_.shape) == spec[name][0] and t_.cpu().numpy().dtype.type == spec[name][1], name
    assert counts["on"].pop("md_traffic_lights") == 6
    assert counts["on"] == counts["off"] and "md_traffic_lights" not in counts["off"]
    assert len(outs["on"]) == len(outs["off"])
    for a, b in zip(outs["on"], outs["off"]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
