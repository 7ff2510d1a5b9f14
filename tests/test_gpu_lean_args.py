"""The lean step kernels fold what their launch pins (csrc/mdstep.hip: lean_pins, the one list that variant<PH_ALL>() tests and that
env_kernel<PH_ALL, false, false, false> and wave_step_kernel<false> overwrite in their by-value arguments).  md_step against
OracleWorld.step, states compared every step:
  the lean path on each of its three kernels with resets from the snapshots and truncation at the horizon,
  the optional fields of the lean path that are NOT pinned, present and absent,
  one neighbour config per pinned field, which must leave the lean kernels and still step bit-exact.
The launch predicate is not reachable from Python (no export), so the neighbours rely on the parity runs."""
import numpy as np
import pytest

from helpers import assert_state_equal, scripted_actions

pytestmark = pytest.mark.gpu

E = 6
LEAN = dict(start_seed=100, traffic_density=0.3, auto_reset=True, horizon=12)


def _pair(**kw):
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    import oracle_binding as ob
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    eng = BatchedEngine(make_config(dict(dict(num_envs=E, num_scenarios=E), **kw)))
    return eng, ob.OracleWorld(eng.host)


def _actions(t):
    a = scripted_actions(E, 1, t, seed=3)
    a[:, :, 0] *= 0.2
    return a


def _rollout(eng, orc, steps, step=None, reset=True):
    """-> resets per env.  `step(eng, a)`: how the engine is stepped (default: eng.step with the caller's tensor)"""
    import torch
    if reset:
        eng.reset()
        orc.reset()
    assert_state_equal(eng.download_state(), orc.state, where="start")
    resets = np.zeros(E, np.int64)
    for t in range(steps):
        a = _actions(t)
        resets += orc.state["need_reset"].reshape(E) != 0
        if step is None:
            eng.step(torch.from_numpy(a).to(eng.device))
        else:
            step(eng, a)
        orc.step(a)
        assert_state_equal(eng.download_state(), orc.state, where="step %d" % t)
    return resets


# ---- the lean path, everything that reads a cold argument: reset snapshots, the reward / done scheme, the lidar ----

@pytest.mark.parametrize("kernel", ["wg", "wg_staged", "wave"])
def test_lean_rollout_with_resets(kernel):
    kw = dict(LEAN)
    if kernel == "wg_staged":
        kw.update(map="S")
    kw.update(step_kernel="wave" if kernel == "wave" else "wg")
    eng, orc = _pair(**kw)
    assert eng.host.step_kernel == kw["step_kernel"]
    assert eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and not eng.k.is_multi_agent
    assert "detected" not in eng.state_dev
    if kernel == "wg":
        assert eng.w.max_lanes > 64, "the batch must take the non-staged workgroup kernel"
    if kernel == "wg_staged":
        assert eng.w.max_lanes <= 64, "the batch must take the staged workgroup kernel"
    resets = _rollout(eng, orc, 60)
    assert (resets >= 1).all(), resets


# ---- optional fields of the lean path that are not pinned ----

def test_actions_through_the_per_slot_array():
    """MdState.agent_action absent: the agents' actions are taken from the per-slot array"""
    eng, orc = _pair(**LEAN)
    assert eng.host.step_kernel == "wg" and eng.w.max_lanes > 64

    def step(eng, a):
        act = np.ascontiguousarray(eng.download_state()["action"])
        act.reshape(E, eng.cap, 2)[:, 0, :] = a[:, 0, :]
        eng.upload_state({"action": act})
        eng.s.agent_action = None
        eng.step_raw()

    assert (_rollout(eng, orc, 30, step=step) >= 1).all()


def test_done_out_absent():
    """MdState.done_out null: nothing is written to the buffer, the step is the same"""
    eng, orc = _pair(**LEAN)
    eng.reset()
    orc.reset()
    before = eng.state_dev["done_out"].clone()
    eng.s.done_out = None
    _rollout(eng, orc, 30, reset=False)
    assert (eng.state_dev["done_out"] == before).all()


def test_done_out_present():
    from metadrive_ped_amd import abi
    eng, orc = _pair(**LEAN)
    import torch
    eng.reset()
    orc.reset()
    seen = 0
    for t in range(30):
        a = _actions(t)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        fl = orc.state["flags"].reshape(E, eng.cap)[:, 0]
        tt = eng.done_tt.cpu().numpy().reshape(E, 2)
        assert (tt[:, 0] == ((fl & abi.FL_TERMINATED) != 0)).all() and (tt[:, 1] == ((fl & abi.FL_TRUNCATED) != 0)).all(), t
        seen += int(tt.any())
    assert seen >= 1


@pytest.mark.parametrize("extra", [dict(random_agent_model=True),
                                   dict(vehicle_config=dict(lidar=dict(num_lasers=0, distance=0))),
                                   dict(vehicle_config=dict(lidar=dict(num_lasers=30, distance=50)))],
                         ids=["random_agent_model", "no_lidar", "lidar_30_beams"])
def test_lean_optional_configs(extra):
    eng, orc = _pair(**dict(LEAN, **extra))
    assert eng.host.step_kernel == "wg" and eng.k.traffic_mode == 0 and "detected" not in eng.state_dev
    assert (_rollout(eng, orc, 30) >= 1).all()


def test_user_spawned_pedestrian():
    """A walking pedestrian in the lean batch (md_walk_mover runs in the lean kernels only)"""
    eng, orc = _pair(**dict(LEAN, horizon=40))
    eng.reset()
    orc.reset()
    ped = eng.spawn_object("pedestrian", [30.0, 0.0], 0.0)
    eng.set_velocity(ped, [1, 0], 1, in_local_frame=True)
    st = eng.download_state()
    for k in ("shape", "shape0", "dyn", "flags"):
        orc.state[k][...] = st[k]
    x0 = eng.object_positions(ped).cpu().numpy().copy()
    _rollout(eng, orc, 30, reset=False)
    assert (np.abs(eng.object_positions(ped).cpu().numpy() - x0).sum(axis=1) > 0.1).all(), "the pedestrian must have walked"


# ---- one neighbour per pinned field: each leaves the lean kernels ----

NEIGHBOURS = [("respawn", dict(traffic_mode="respawn")),
              ("hybrid", dict(traffic_mode="hybrid")),
              ("idm_policy", dict(agent_policy="IDMPolicy")),
              ("num_others_4", dict(vehicle_config=dict(lidar=dict(num_others=4))))]


@pytest.mark.parametrize("extra", [n[1] for n in NEIGHBOURS], ids=[n[0] for n in NEIGHBOURS])
def test_neighbour_of_a_pinned_field(extra):
    eng, orc = _pair(**dict(LEAN, **extra))
    pinned = eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and "detected" not in eng.state_dev
    assert not pinned, "the neighbour config must break a pin"
    _rollout(eng, orc, 30)


def test_neighbour_lane_change_policy():
    """agent_policy LaneChangePolicy: the oracle is driven by the host restatement of include/md_lane_change.h (tests/lane_change_host.py),
    whose PID errors stand in the agents' rows"""
    import torch
    import lane_change_host as lh
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    eng = BatchedEngine(make_config(dict(LEAN, num_envs=E, num_scenarios=E, agent_policy="LaneChangePolicy", discrete_action=True)))
    assert eng.k.agent_idm == abi.AGENT_LANE_CHANGE
    lc = lh.LaneChangeOracle(eng.host)

    def expected():
        ref = {k: v.copy() for k, v in lc.state.items()}
        rows = lc.agent_rows()
        for k in lh.PID_ERRS:
            ref["pid"][k][rows] = lc.pid[k][rows]
        return ref

    eng.reset()
    lc.reset()
    assert_state_equal(eng.download_state(), expected(), where="reset")
    rng = np.random.RandomState(5)
    for t in range(30):
        d = np.zeros((E, 1, 2), np.float32)
        d[..., 0] = rng.randint(-1, 2, (E, 1))
        d[..., 1] = rng.choice(np.float32([-0.5, 0.0, 0.5, 1.0]), (E, 1))
        eng.step(torch.from_numpy(d).to(eng.device))
        lc.step(d)
        assert_state_equal(eng.download_state(), expected(), where="step %d" % t)


def test_neighbour_replay():
    """traffic_mode replay: the recorded traffic of the lean batch's own rollout"""
    import torch
    import oracle_binding as ob
    _, rec = _pair(**LEAN)
    rec.reset()
    tracks = ob.record_episode(rec, [_actions(t) for t in range(12)])
    eng, orc = _pair(**dict(LEAN, traffic_mode="replay"))
    assert eng.k.traffic_mode == 3
    eng.set_tracks(dict(tracks, shape=torch.from_numpy(tracks["shape"].view(np.uint8).reshape(len(tracks["shape"]), -1)),
                        dyn=torch.from_numpy(tracks["dyn"])))
    orc.set_tracks(tracks["shape"], tracks["dyn"])
    _rollout(eng, orc, 30)
