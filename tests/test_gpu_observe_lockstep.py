"""The agent's observation of the lean step kernel with its nine tasks in lock-step (csrc/parts/observe.inc: observe_agent_wave1<true>,
include/md_entity.h: md_observe_lane) against the oracle, which runs the serial tasks (md_observe_task): md_step rollouts with
resets, horizon truncations, out-of-road terminations, both directions of circular lanes and road boundaries, every step's
observation row before the cloud, reward, cost, terminated / truncated, step flags and step_info bit for bit."""
import numpy as np
import pytest

from helpers import assert_state_equal

E = 8
SLOT = 0
STEPS = 120
RANDOM_ENVS = (3, 6)     # act at random and leave the road; the other six follow their lanes across road boundaries
CONFIG = dict(num_envs=E, num_scenarios=E, start_seed=5000, traffic_density=0.3, auto_reset=True, horizon=60)
OUTPUTS = ("reward", "cost", "done_out", "flags", "step_info")


def _events(host, state, resetting):
    """What the oracle's state shows after a step -> the set of event names (the agents' slots only)"""
    from metadrive_ped_amd import abi
    cap = host.cap
    rows = np.arange(E) * cap + SLOT
    out = set()
    if resetting.any():
        out.add("reset step")
    fl = state["flags"][rows]
    done = state["done_out"].reshape(E, -1, 4)[:, 0]
    if ((fl & abi.FL_MAX_STEP) != 0).any() and (done[:, 1] != 0).any():
        out.add("horizon truncation")
    if (((fl & abi.FL_OUT_OF_ROAD) != 0) & (done[:, 0] != 0)).any():
        out.add("out-of-road termination")
    arr = host.world.arrays
    for e in range(E):
        lane = int(state["nav"]["lane"][rows[e]])
        if lane < 0:
            continue
        rec = arr["lanes"][int(arr["lane_off"][int(arr["env_map"][e])]) + lane]
        if rec["type"] == 1:
            out.add("circular lane, counter-clockwise" if rec["dirsign"] > 0 else "circular lane, clockwise")
        if int(rec["road"]) != int(state["nav"]["road0"][rows[e]]):
            out.add("lane.road != nav.road0")
    return out


NEEDED = {"reset step", "horizon truncation", "out-of-road termination", "circular lane, counter-clockwise", "circular lane, clockwise",
          "lane.road != nav.road0"}


CRUISE = 24.0            # m/s: the first block is straight, and an episode is 60 steps of 0.1 s


def _actions(orc, host, t):
    """Six agents steer along their current lane at CRUISE (they reach the curved blocks and cross road boundaries within the
    horizon); RANDOM_ENVS act at random and leave the road"""
    import math
    a = np.zeros((E, 1, 2), np.float32)
    env_map = host.world.arrays["env_map"]
    rng = np.random.RandomState(977 + t)
    for e in range(E):
        n = e * host.cap + SLOT
        if e in RANDOM_ENVS:
            a[e, 0] = rng.uniform(-1, 1, 2)
            a[e, 0, 1] = abs(a[e, 0, 1])
            continue
        sh, l = orc.state["shape"][n], int(orc.state["nav"]["lane"][n])
        steer = 0.0
        if l >= 0:
            lane = host.map_tables[int(env_map[e])].lane_objs[l]
            s, lat = lane.local_coordinates((float(sh["cx"]), float(sh["cy"])))
            err = math.atan2(float(sh["s"]), float(sh["c"])) - lane.heading_theta_at(min(max(s, 0.0), lane.length))
            err = (err + math.pi) % (2 * math.pi) - math.pi
            steer = max(-1.0, min(1.0, 0.3 * lat + 1.5 * err))    # lat > 0: right of the centre line, so steer left (positive)
        a[e, 0] = (steer, 1.0 if float(orc.state["dyn"]["speed"][n]) < CRUISE else 0.0)
    return a


def oracle_rollout(config, steps=STEPS, eng=None):
    """The oracle alone (eng None: no GPU) or md_step beside it, compared every step -> the events the rollout contained"""
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    import oracle_binding as ob
    if eng is None:
        host = HostScene(make_config(config))
    else:
        import torch
        host = eng.host
    orc = ob.OracleWorld(host)
    orc.reset()
    if eng is not None:
        eng.reset()
    n_state = orc.state["obs"].shape[-1] - int(host.md_config.n_beams)    # the dims before the cloud
    seen = set()
    for t in range(steps):
        a = _actions(orc, host, t)
        resetting = orc.state["need_reset"].reshape(E) != 0
        orc.step(a)
        seen |= _events(host, orc.state, resetting)
        if eng is not None:
            eng.step(torch.from_numpy(a).to(eng.device))
            got = eng.download_state()
            g, r = got["obs"].reshape(E, -1)[:, :n_state], orc.state["obs"].reshape(E, -1)[:, :n_state]
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), "step %d: obs before the cloud differs in envs %r" % (
                t, np.nonzero((g.view(np.uint32) != r.view(np.uint32)).any(axis=1))[0].tolist())
            assert_state_equal(got, orc.state, keys=OUTPUTS, where="step %d" % t)
            assert_state_equal(got, orc.state, where="step %d (whole state)" % t)
    return seen


def _engine(config):
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    eng = BatchedEngine(make_config(config))
    assert eng.host.step_kernel == "wg" and eng.w.max_lanes > 64, "the batch must take the lean, non-staged workgroup kernel"
    return eng


@pytest.mark.gpu
def test_rollout_with_traffic():
    seen = oracle_rollout(CONFIG, eng=_engine(CONFIG))
    assert NEEDED <= seen, "the rollout lacks %r" % sorted(NEEDED - seen)


@pytest.mark.gpu
def test_rollout_no_traffic():
    """traffic_density 0: wave 0 is the env's critical wave"""
    cfg = dict(CONFIG, traffic_density=0.0)
    seen = oracle_rollout(cfg, eng=_engine(cfg))
    assert {"reset step", "horizon truncation"} <= seen, sorted(seen)


def test_seeds_show_every_event_on_the_oracle():
    """The chosen seeds and actions, on the oracle alone: the rollout the GPU test compares contains every event it asserts"""
    seen = oracle_rollout(CONFIG)
    assert NEEDED <= seen, "the rollout lacks %r" % sorted(NEEDED - seen)
