"""The lean non-staged workgroup kernels store each slot from the wave that finished it (include/md_write_back_own.h; csrc/mdstep.hip:
MD_WRITE_BACK_OWN): wave 0 the agent's slot behind its observe, an IDM wave a traffic vehicle's behind its decision, the last
wave the removed slots and the walkers; only a reset step keeps the last barrier and the full write-back.  A store that is lost
shows in HBM one step before it shows in an output, so every case here compares the WHOLE state with OracleWorld.step after EVERY
step (assert_state_equal, all arrays), on the placed scenes of tests/test_gpu_size_pins.py: 8 envs, 30 beams, a dozen or two steps.

One case per class of slot that can be lost.  Each asserts ON THE ORACLE'S OWN STATES that the event it is named for happened in
the compared window; trace(..., step_engine=False) runs the oracle alone, which is how the scenes were chosen on the CPU.

A walking participant (case 7): a lean batch does take these kernels with one -- md_walk_mover is part of their integrate stage --
so the case is here (the walker is spawned as tests/test_gpu_ped.py spawns its user participant, with no pedestrian policy)."""
import numpy as np
import pytest

import test_gpu_size_pins as sp
from helpers import assert_state_equal
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

E = sp.E


def _assert_lean_non_staged(eng, cap):
    lean = eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and not eng.k.is_multi_agent and "detected" not in eng.state_dev
    assert lean and eng.host.step_kernel == "wg" and eng.w.max_lanes > 64 and eng.cap == cap and eng.k.agents_per_env == 1, \
        "the batch must take the lean, non-staged workgroup kernel"


def trace(cap, targets, wake, steps, events=None, actions=sp.actions, step_engine=True, seed=None):
    """md_step against the oracle over `steps` steps of sp.build_host's scene, the whole state compared after every step.
    events(t, state) -> keys it changed in the oracle's state before step t (uploaded to the engine).
    seed: the scene's start seed in place of sp.SEED.
    -> per step: the shape flags [E, cap] before and after it, need_reset [E] before and after it (the oracle's)"""
    import oracle_binding as ob
    keep = sp.SEED
    try:
        sp.SEED = keep if seed is None else seed      # build_host reads it when called
        cfg, host = sp.build_host(cap, targets, wake, None)
    finally:
        sp.SEED = keep
    orc = ob.OracleWorld(host)
    eng = None
    if step_engine:
        import torch
        from metadrive_ped_amd.engine import BatchedEngine
        assert torch.cuda.is_available(), "GPU tests need a ROCm device"
        eng = BatchedEngine(cfg, host=host)
        _assert_lean_non_staged(eng, cap)
        eng.reset()
    orc.reset()
    if eng is not None:
        assert_state_equal(eng.download_state(), orc.state, where="cap %d start" % cap)
    f0, f1, r0, r1 = [], [], [], []
    for t in range(steps):
        keys = events(t, orc.state) if events else None
        if keys and eng is not None:
            eng.upload_state({k: orc.state[k] for k in keys})
        f0.append(orc.state["shape"]["flags"].reshape(E, cap).copy())
        r0.append(orc.state["need_reset"].reshape(E).copy())
        a = actions(t)
        if eng is not None:
            eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        if eng is not None:
            assert_state_equal(eng.download_state(), orc.state, where="cap %d step %d" % (cap, t))
        f1.append(orc.state["shape"]["flags"].reshape(E, cap).copy())
        r1.append(orc.state["need_reset"].reshape(E).copy())
    return np.asarray(f0), np.asarray(f1), np.asarray(r0), np.asarray(r1)


def traffic_driving(flags):
    return sp.drives(flags) & ((flags & abi.F_AGENT) == 0)


def push_off(env, slot, at):
    """before step `at`: the vehicle in `slot` of `env` 600 m off every lane (the step removes it)"""
    def events(t, state):
        if t != at:
            return None
        n = env * (len(state["shape"]) // E) + slot
        assert sp.drives(state["shape"]["flags"][n:n + 1])[0], "the vehicle to remove must drive"
        for k, last_k in (("cx", "last_x"), ("cy", "last_y")):
            state["shape"][k][n] += np.float32(600.0)
            state["dyn"][last_k][n] += np.float32(600.0)
        return ("shape", "dyn")
    return events


# ---- 1: only the agent drives ----
def check_agent_alone(step_engine=True):
    f0, f1, r0, _ = trace(16, (), 0, 6, step_engine=step_engine)
    assert not r0.any()
    assert (sp.drives(f0).sum(axis=2) == 1).all() and sp.drives(f0)[:, :, 0].all(), "the agent and nothing else drives"


def test_only_the_agent_drives():
    check_agent_alone()


# ---- 2: a trigger fires ----
TRIGGER_STEPS = 27          # in these scenes the first trigger road is reached in step 23


def check_trigger(step_engine=True):
    f0, f1, r0, _ = trace(16, (), 0, TRIGGER_STEPS, step_engine=step_engine)
    woken = ((f0 & abi.F_PENDING) != 0) & ((f1 & abi.F_PENDING) == 0) & ~(r0 != 0)[:, :, None]
    assert woken[:-2].any(), "a trigger must fire at least two steps before the end: the woken slots' first plan and first move are compared"
    t, e, j = [int(x[0]) for x in np.nonzero(woken)]
    assert sp.drives(f1[t, e, j:j + 1])[0] and traffic_driving(f0[t + 1, e])[j], "the woken vehicle drives in the next step"
    return woken


def test_a_trigger_fires():
    check_trigger()


# ---- 3: a traffic vehicle leaves its lane and is removed ----
def check_removed(step_engine=True):
    env, slot, at = 2, 15, 5
    f0, f1, r0, _ = trace(16, (slot, ), 1, 10, events=push_off(env, slot, at), step_engine=step_engine)
    assert not r0[at].any()
    assert sp.drives(f0[at, env, slot:slot + 1])[0] and not (f1[at, env, slot] & abi.F_ALIVE), "step %d must remove the vehicle" % at
    assert not (f1[at + 1:, env, slot] & abi.F_ALIVE).any()
    assert sp.drives(f0[:, [x for x in range(E) if x != env], slot]).all(), "the other envs keep theirs"


def test_a_traffic_vehicle_is_removed():
    check_removed()


# ---- 4: more driving traffic vehicles than IDM waves ----
MANY = {4: sp.SEED, 6: 5002}   # wake -> start seed: of sp.SEED's eight scenes one parks only four vehicles; 5002's all park six or more


def check_many(wake, step_engine=True):
    f0, f1, r0, _ = trace(24, (23, ), wake, 10, step_engine=step_engine, seed=MANY[wake])
    assert not r0.any()
    n = traffic_driving(f0).sum(axis=2)
    assert (n[:3] >= wake).all(), "%d traffic vehicles must drive from the start: %r" % (wake, n[:3].tolist())
    assert traffic_driving(f0)[:, :, 23].all()


@pytest.mark.parametrize("wake", [4, 6])
def test_one_wave_plans_two_vehicles(wake):
    """three IDM waves: with four driving traffic vehicles one wave plans two, with six every wave does"""
    check_many(wake)


# ---- 5: an episode ends: the step that ends it, the reset step, the step after ----
ENV_OFF = 3
END_STEPS = 20              # the veering agent is off the road in step 15


def veer(t):
    a = sp.actions(t)
    a[ENV_OFF, 0, 0] = 1.0        # hard over: off the road
    a[ENV_OFF, 0, 1] = 1.0
    return a


def check_episode_ends(step_engine=True):
    f0, f1, r0, r1 = trace(16, (15, ), 1, END_STEPS, actions=veer, step_engine=step_engine)
    ends = np.nonzero((r0[:, ENV_OFF] == 0) & (r1[:, ENV_OFF] != 0))[0]
    assert len(ends) >= 1 and ends[0] + 2 < END_STEPS, "env %d must end its episode two steps before the rollout's end: %r" % (ENV_OFF, ends.tolist())
    t = int(ends[0])
    assert r0[t + 1, ENV_OFF] != 0 and r1[t + 1, ENV_OFF] == 0, "step %d is the reset step" % (t + 1)
    assert r0[t + 2, ENV_OFF] == 0 and sp.drives(f0[t + 2, ENV_OFF, 0:1])[0], "the env drives again in step %d" % (t + 2)
    others = [x for x in range(E) if x != ENV_OFF]
    assert not r0[t:t + 3, others].any(), "the other envs step on beside the reset (block-uniform per env, not per launch)"


def test_an_episode_ends_and_the_env_resets():
    check_episode_ends()


# ---- 6: the last mask bit of the narrow kernel; the second mask word of its sibling ----
def check_slot_63(step_engine=True):
    f0, f1, r0, _ = trace(64, (63, 40), 2, 8, step_engine=step_engine)
    assert not r0.any() and traffic_driving(f0)[:, :, 63].all() and traffic_driving(f0)[:, :, 40].all()


def test_cap_64_slot_63_drives():
    check_slot_63()


def check_cap_72(step_engine=True):
    env, at = 2, 4
    f0, f1, r0, _ = trace(72, (71, 66), 2, 9, events=push_off(env, 71, at), step_engine=step_engine)
    assert not r0.any()
    assert traffic_driving(f0)[:, :, 66].all(), "slot 66 drives in every step of every env"
    assert traffic_driving(f0)[:at + 1, :, 71].all()
    assert not (f1[at, env, 71] & abi.F_ALIVE), "step %d must remove slot 71 of env %d" % (at, env)


def test_cap_72_slots_above_64_drive_and_are_removed():
    check_cap_72()


# ---- 7: a walking participant in a lean batch ----
def test_a_walker_in_a_lean_batch():
    import oracle_binding as ob
    from helpers import scripted_actions
    from metadrive_ped_amd import participants as P
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    cap = 32
    env = BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=E, start_seed=sp.SEED, traffic_density=0.1, mover_capacity=cap, horizon=1000,
                                   vehicle_config=dict(lidar=dict(num_lasers=30, distance=50))))
    env.reset()
    eng = env.engine
    _assert_lean_non_staged(eng, cap)
    orc = ob.OracleWorld(eng.host)
    orc.reset()
    at = eng.shape_f[:, 0, 0:2].cpu().numpy() + np.float32([12.0, 6.0])
    slot = env.spawn_object("pedestrian", at, heading_theta=0.5)
    env.set_velocity(slot, [1, 0], 1.4, in_local_frame=True)
    assert slot == P.spawn(orc.state, E, cap, 1, "pedestrian", at, heading_theta=0.5)
    P.set_velocity(orc.state, E, cap, slot, [1, 0], 1.4, in_local_frame=True)
    assert_state_equal(eng.download_state(), orc.state, where="walker start")
    where0 = orc.state["shape"].reshape(E, cap)[:, slot][["cx", "cy"]].copy()
    for t in range(10):
        a = scripted_actions(E, 1, t)
        assert not orc.state["need_reset"].any()
        fl = orc.state["shape"]["flags"].reshape(E, cap)[:, slot]
        assert ((fl & abi.KIND_MASK) == abi.KIND_PEDESTRIAN).all() and ((fl & abi.F_ALIVE) != 0).all() and ((fl & abi.F_STATIC) == 0).all(), "it walks"
        env.step(a[:, 0])
        orc.step(a)
        assert_state_equal(eng.download_state(), orc.state, where="walker step %d" % t)
    now = orc.state["shape"].reshape(E, cap)[:, slot]
    moved = np.hypot(now["cx"] - where0["cx"], now["cy"] - where0["cy"])
    assert (moved > 1.0).all(), "the walker walked in the oracle: %r" % moved.tolist()
