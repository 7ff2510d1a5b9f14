"""The vector scene observation on the MI355X (md_vector_obs, include/md_vector_obs.h): env.vector_obs() and the engine-owned
history bit for bit against the gcc host build of the header (tests/vector_obs_host.py), run on the state downloaded after every
step; every env family and traffic mode the kernel has a path for; snapshots; the walk; one launch per step."""
import numpy as np
import pytest

import vector_obs_host as vh
from helpers import scripted_actions
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

PG = dict(num_envs=8, num_scenarios=8, map="CXO", traffic_density=0.3, horizon=12, vector_obs=dict(vh.SMALL))


def _env_map(env):
    return env.engine.world_dev["env_map"].view(env.engine.torch.int32).cpu().numpy().copy()


class Parity:
    """The host build stepped beside the device: its own history rows, fed the state the device's launch read"""
    def __init__(self, env):
        self.env, self.eng = env, env.engine
        h = self.eng.host
        self.hv = vh.HostVectorObs(env.config["vector_obs"], h.E, h.A, h.cap)
        self.before = None       # a walking batch: the env maps and route constants as they were before the step's swap

    def device_outputs(self):
        out = self.env.vector_obs()
        if not self.env.config["is_multi_agent"]:
            out = {k: t.unsqueeze(1) for k, t in out.items()}
        return {k: t.cpu().numpy() for k, t in out.items()}

    def check(self, where, walk=False):
        state = self.eng.download_state()
        env_map = _env_map(self.env)
        seen = dict(state)
        if walk and self.before is not None:     # the launch came before md_swap_draw moved the ended envs on
            seen.update(self.before[1])
        w, s, k, keep = vh.structs_of(self.eng.host, seen, self.before[0] if walk and self.before is not None else env_map)
        self.hv.run(w, s, k)
        self.before = (env_map, {n: state[n].copy() for n in ("route_roads", "final_lane", "route_nodes")})
        dev, want = self.device_outputs(), self.hv.outputs()
        assert list(dev) == list(abi.VECTOR_OBS_OUTPUTS)
        for name in abi.VECTOR_OBS_OUTPUTS:
            assert dev[name].shape == want[name].shape and dev[name].dtype == want[name].dtype, (where, name)
            if dev[name].tobytes() != want[name].tobytes():
                bad = np.argwhere(dev[name] != want[name])[:4]
                raise AssertionError("%s: %s differs at %s: device %s, host %s" % (where, name, bad.tolist(), [dev[name][tuple(i)] for i in bad],
                                                                                 [want[name][tuple(i)] for i in bad]))
        hist, want_hist = self.eng.vector_obs_history(), self.hv.history()
        for name in abi.VECTOR_OBS_HISTORY:
            assert hist[name].tobytes() == want_hist[name].tobytes(), (where, name)
        return dev, state


def _pg(**kw):
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    return BatchedMetaDriveEnv(dict(PG, **kw))


def _drive(E, t):
    """scripted actions whose every env drives (env 0 of helpers.scripted_actions brakes)"""
    return scripted_actions(E + 1, 1, t)[1:, 0]


# -- 1. single-agent envs: traffic modes x step kernels, envs resetting themselves inside the run --------------------------------
@pytest.mark.parametrize("step_kernel", ["wg", "wave"])
@pytest.mark.parametrize("traffic_mode", ["trigger", "respawn"])
def test_bit_exact_against_the_host_build(traffic_mode, step_kernel):
    env = _pg(traffic_mode=traffic_mode, step_kernel=step_kernel)
    env.reset()
    assert env.engine.host.step_kernel == step_kernel
    p = Parity(env)
    dev, _ = p.check("reset")
    assert (p.hv.history()["cursor"][:, 1] == 1).all() and dev["ego_mask"][:, 0].tolist() == [[1, 0, 0]] * 8
    resets, full, neighbours = 0, 0, 0
    for t in range(25):
        env.step(_drive(8, t))
        dev, state = p.check("step %d" % t)
        held = p.hv.history()["cursor"][:, 1]
        resets += int((held == 1).sum())
        full += int((held == 3).sum())
        neighbours += int(dev["agents_mask"][:, 0, :, 0].sum())
    assert resets >= 8 and full >= 8 and neighbours > 0, (resets, full, neighbours)


def test_default_shapes():
    env = _pg(vector_obs={}, num_envs=16, num_scenarios=16, horizon=30)
    env.reset()
    p = Parity(env)
    p.check("reset")
    for t in range(8):
        env.step(_drive(16, t))
        dev, _ = p.check("step %d" % t)
    assert {k: tuple(v.shape) for k, v in env.vector_obs().items()} == {k: s for k, (s, _) in env.vector_obs_spec().items()}
    assert all(t.device.type == "cuda" for t in env.vector_obs().values())
    assert dev["route_mask"].any() and dev["lanes_mask"].all() and dev["ego_mask"][:, 0, :].all()


# -- 2. multi-agent: observers share the env's push; slots respawn -----------------------------------------------------------------
def _marl_actions(E, A, t):
    a = scripted_actions(E + 1, A, t)[1:].copy()
    a[:, ::5, 0] = 0.9         # every fifth agent leaves the road: its slot is respawned delay_done steps later
    return a


def test_multi_agent_intersection():
    from metadrive_ped_amd.envs import BatchedMultiAgentIntersectionEnv
    env = BatchedMultiAgentIntersectionEnv(dict(num_envs=2, delay_done=3, vector_obs=dict(vh.SMALL, radius=16.0, route_spacing=10.0)))
    env.reset()
    p = Parity(env)
    _, state = p.check("reset")
    ids, A = state["agent_id"].copy(), env.config["num_agents"]
    invalid = 0
    for t in range(25):
        env.step(_marl_actions(2, A, t))
        dev, state = p.check("step %d" % t)
        invalid += int((dev["ego_mask"][:, :, 0] == 0).sum())
    assert (state["agent_id"] != ids).sum() >= 2, "the run must respawn agents in their slots"
    assert invalid > 0 and dev["agents_mask"].any() and dev["route_mask"].any()


# -- 3. pedestrians and a user-spawned cyclist are neighbours, with their kinds -----------------------------------------------------
def test_pedestrians_and_a_cyclist_are_neighbours():
    env = _pg(num_envs=4, num_scenarios=4, map="SCX", traffic_density=0.0, horizon=1000, num_pedestrians=2,
              vector_obs=dict(vh.SMALL, radius=1000.0))
    env.reset()
    p = Parity(env)
    p.check("reset")            # the reset frame holds no cyclist yet
    start = env.engine.shape_f[:, 0, 0:2].cpu().numpy()
    bike = env.spawn_object("cyclist", (start + np.asarray([12.0, 6.0], np.float32)).tolist(), 0.0)     # beside the road: never hit
    env.set_velocity(bike, [1, 0], 3.0, in_local_frame=True)
    for t in range(6):
        env.step(_drive(4, t))
        dev, _ = p.check("step %d" % t)
        kinds = np.sort(dev["agents_meta"][:, 0, :, 3], axis=1)
        assert kinds.tolist() == [[float(abi.KIND_PEDESTRIAN)] * 2 + [float(abi.KIND_CYCLIST)]] * 4, (t, kinds)
        bikes = dev["agents_meta"][:, 0, :, 3] == float(abi.KIND_CYCLIST)
        assert dev["agents_mask"][:, 0][bikes].tolist() == [[1] + [int(t >= k) for k in (1, 2)]] * 4, t   # its history starts at the spawn
    assert dev["agents_mask"][:, 0].all(), "three frames of every walker"


# -- 4. more than 64 slots: two slots per lane ----------------------------------------------------------------------------------
def test_capacity_above_64():
    env = _pg(num_envs=2, num_scenarios=2, accident_prob=1.0, traffic_density=0.05, mover_capacity=72, horizon=1000,
              vector_obs=dict(vh.SMALL, num_agents=16, radius=1000.0))
    env.reset()
    assert env.engine.cap == 72
    p = Parity(env)
    p.check("reset")
    flags = env.engine.download_state()["shape"]["flags"].reshape(2, 72)
    assert ((flags[:, 64:] & abi.F_ALIVE) != 0).any(), "the accident scenes' props sit in the top slots"
    props = 0
    for t in range(8):
        env.step(_drive(2, t))
        dev, _ = p.check("step %d" % t)
        props += int((dev["agents_meta"][:, 0, :, 3] >= abi.KIND_CONE).sum())
    assert props > 0, "props from the slots above 64 must be among the neighbours"


# -- 5. snapshots carry the history and the observation ---------------------------------------------------------------------------
def _obs_bytes(env):
    out = {k: t.cpu().numpy().copy() for k, t in env.vector_obs().items()}
    out.update(env.engine.vector_obs_history())
    return out


def test_branch_and_snapshot_carry_the_history():
    env = _pg(horizon=40)
    env.reset()
    for t in range(6):
        env.step(_drive(8, t))
    env.branch(0, [1, 2])
    now = _obs_bytes(env)
    for k, v in now.items():
        assert v[1].tobytes() == v[0].tobytes() and v[2].tobytes() == v[0].tobytes(), k      # the current observation travels too
    a = _drive(8, 6)
    a[1:3] = a[0]
    env.step(a)
    now = _obs_bytes(env)
    for k, v in now.items():
        assert v[1].tobytes() == v[0].tobytes() and v[2].tobytes() == v[0].tobytes(), k
    assert now["ego_mask"][1].tolist() == [1, 1, 1], "the history came along: three valid frames right after the branch"
    snap = env.snapshot()
    first = []
    for t in range(7, 11):
        env.step(_drive(8, t))
        first.append(_obs_bytes(env))
    env.restore(snap)
    back = _obs_bytes(env)
    assert all(back[k].tobytes() == now[k].tobytes() for k in now)
    for i, t in enumerate(range(7, 11)):
        env.step(_drive(8, t))
        again = _obs_bytes(env)
        assert all(again[k].tobytes() == first[i][k].tobytes() for k in again), t


def test_set_state_forgets_the_history():
    env = _pg(horizon=40)
    env.reset()
    for t in range(4):
        env.step(_drive(8, t))
    st = env.get_state()
    assert not any("vector" in k for k in st)
    env.set_state(st)
    assert not env.engine.vector_obs_history()["cursor"].any()
    env.step(_drive(8, 4))
    assert env.vector_obs()["ego_mask"].cpu().numpy().tolist() == [[1, 0, 0]] * 8


# -- 6. the walk: the step that ends an episode is traced on the old map ---------------------------------------------------------------
def test_a_walking_env_s_last_frame_is_traced_on_the_old_map():
    env = _pg(walk_scenarios=True, num_envs=6, num_scenarios=10, map=2, traffic_density=0.15, horizon=8, start_seed=30)
    env.reset()
    p = Parity(env)
    p.check("reset", walk=True)
    moved = 0
    for t in range(20):
        maps_before = _env_map(env)
        env.step(_drive(6, t))
        dev, state = p.check("step %d" % t, walk=True)       # the host build runs on the maps as they were before the swap
        maps_after = _env_map(env)
        arr = env.engine.host.world.arrays
        for e in np.nonzero(maps_after != maps_before)[0]:
            moved += 1
            # explicitly: the lanes the device reported for the step that ended the episode are lanes of the OLD map
            m = int(maps_before[e])
            table = arr["lanes"][int(arr["lane_off"][m]):int(arr["lane_off"][m + 1])]
            taken = dev["lanes_mask"][e, 0] != 0
            assert taken.any() or not dev["ego_mask"][e, 0, 0]
            for width, length in dev["lanes_meta"][e, 0][taken][:, :2]:
                assert ((table["width"] == width) & (table["length"] == length)).any(), (t, e)
    assert moved >= 3, "envs must end episodes and move on to other maps inside the run"


# -- 7. one launch per step, none without the key ----------------------------------------------------------------------------------
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
    for key, vo in (("on", dict(vh.SMALL)), ("off", None)):
        env = _pg(vector_obs=vo, horizon=40)
        env.reset()
        lib = env.engine.lib = _CountingLib(env.engine.lib)
        for t in range(5):
            env.step(_drive(8, t))
        counts[key] = dict(lib.calls)
        if vo is None:
            assert env.engine.vector_obs_rows is None and env.engine.vector_obs_hist is None
            with pytest.raises(RuntimeError, match="vector_obs"):
                env.vector_obs()
    assert counts["on"].pop("md_vector_obs") == 5
    assert counts["on"] == counts["off"] and "md_vector_obs" not in counts["off"]
