"""The size pins of the lean launch (include/md_lean_pins.h: one agent per env, at most 64 mover slots): a lean batch that holds
them takes the narrow form of the lean non-staged step kernel (csrc/mdstep.hip: env_kernel<PH_ALL, false, false, false, BLK, true>),
one that does not (capacity 65, 72) keeps the lean kernel.  md_step against OracleWorld.step on PLACED scenes of 8 envs with 30 beams
over about 20 steps, the whole state compared after every step.

A scene is the host scene of the config with its slots permuted before anything is uploaded (every per-slot array, live and
snapshot, so resets restore the same placement): two parked traffic vehicles go to the LAST slot of the scene (63 at capacity 64:
the last mask bit) and to slot 40 (>= 32: a 32-bit shift would lose it) and are woken, a cone stands in slot 50 between them.  In the
middle of the rollout the last-slot vehicle of one env is put far off every lane (the step removes it: the dirty write-back of the
last slot) and another env is told to reset.  The coverage is asserted from the oracle's states, not assumed.

Which kernel ran is not visible from Python (the library reports none): tests/test_lean_pins_host.py pins the predicate, and
profiles/size_pins_ab.txt holds the kernel trace taken by hand."""
import numpy as np
import pytest

import test_gpu_contacts as tc
from helpers import assert_state_equal
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

E = 8
STEPS = 20
T_PLACE = 8            # the step before which the removal and the reset are placed
ENV_REMOVE, ENV_RESET = 2, 5
SEED = 5000


def drives(flags):
    return ((flags & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((flags & abi.F_ALIVE) != 0) & ((flags & (abi.F_STATIC | abi.F_PENDING)) == 0)


def _parked(flags):
    return np.nonzero(((flags & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((flags & abi.F_ALIVE) != 0) & ((flags & abi.F_PENDING) != 0) &
                      ((flags & (abi.F_AGENT | abi.F_STATIC)) == 0))[0]


def build_host(cap, targets, wake, cone_slot=None):
    """-> the host scene of the config at capacity `cap`; in every env the first len(targets) parked traffic vehicles moved to the
    slots `targets` and `wake` parked vehicles awake in all (the moved ones first); a cone in `cone_slot`"""
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    cfg = make_config(dict(num_envs=E, num_scenarios=E, start_seed=SEED, traffic_density=0.1, mover_capacity=cap, auto_reset=True, horizon=1000,
                           vehicle_config=dict(lidar=dict(num_lasers=30, distance=50))))
    host = HostScene(cfg)
    assert host.cap == cap and host.A == 1 and host.E == E
    st = host.state
    N = E * cap
    per_slot = [k for k, v in st.items() if v.shape[0] == N]
    assert {"shape", "shape0", "dyn", "dyn0", "nav", "nav0", "pid", "pid0", "param", "route_nodes", "route_roads", "final_lane", "action",
            "flags"} <= set(per_slot)
    for e in range(E):
        f = st["shape0"]["flags"][e * cap:(e + 1) * cap]
        parked = _parked(f)
        assert len(parked) >= max(wake, len(targets)), "env %d parks %d vehicles" % (e, len(parked))
        perm = np.arange(cap)
        for src, dst in zip(parked, targets):
            assert (f[dst] & abi.F_ALIVE) == 0 and (f[dst] & abi.KIND_MASK) == abi.KIND_NONE, "slot %d of env %d is taken" % (dst, e)
            perm[dst], perm[src] = src, dst
        for k in per_slot:
            st[k][e * cap:(e + 1) * cap] = st[k][e * cap:(e + 1) * cap][perm].copy()
        f = st["shape0"]["flags"][e * cap:(e + 1) * cap]
        awake = list(targets) + [int(j) for j in _parked(f) if j not in targets]
        for j in awake[:wake]:
            for k in ("shape", "shape0"):
                st[k]["flags"][e * cap + j] &= ~np.uint32(abi.F_PENDING)
        if cone_slot is not None:
            me = st["shape0"][e * cap]
            assert (f[cone_slot] & abi.F_ALIVE) == 0
            ctr = (float(me["cx"]) + 10.0 * float(me["c"]) - 5.0 * float(me["s"]), float(me["cy"]) + 10.0 * float(me["s"]) + 5.0 * float(me["c"]))
            cone = tc._body("cone", ctr, 0.0)
            for k in ("shape", "shape0"):
                st[k][e * cap + cone_slot] = cone
    return cfg, host


def actions(t):
    a = np.zeros((E, 1, 2), np.float32)
    a[:, 0, 1] = 0.6
    a[:, 0, 0] = 0.02 * np.sin(0.3 * t + np.arange(E))
    return a


def place_events(state, cap, last):
    """before step T_PLACE: the last-slot vehicle of ENV_REMOVE 600 m off (no lane there), ENV_RESET told to reset -> the keys written"""
    n = ENV_REMOVE * cap + last
    assert drives(state["shape"]["flags"][n:n + 1])[0], "the vehicle to remove must drive"
    for k, last_k in (("cx", "last_x"), ("cy", "last_y")):
        state["shape"][k][n] += np.float32(600.0)
        state["dyn"][last_k][n] += np.float32(600.0)
    state["need_reset"][ENV_RESET] = 1
    return ("shape", "dyn", "need_reset")


def rollout(cap, targets, wake, cone_slot, events, step_engine=True):
    """-> coverage: per step the driving mask [E, cap] before the step, the removal, the reset.  step_engine=False: the oracle alone"""
    import oracle_binding as ob
    cfg, host = build_host(cap, targets, wake, cone_slot)
    orc = ob.OracleWorld(host)
    eng = None
    if step_engine:
        import torch
        from metadrive_ped_amd.engine import BatchedEngine
        assert torch.cuda.is_available(), "GPU tests need a ROCm device"
        eng = BatchedEngine(cfg, host=host)
        lean = eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and not eng.k.is_multi_agent and "detected" not in eng.state_dev
        assert lean and eng.host.step_kernel == "wg" and eng.w.max_lanes > 64 and eng.cap == cap and eng.k.agents_per_env == 1, \
            "the batch must take the lean, non-staged workgroup kernel"
        eng.reset()
    orc.reset()
    if eng is not None:
        assert_state_equal(eng.download_state(), orc.state, where="cap %d start" % cap)
    last = max(targets)
    drove, removed, reset_seen = [], False, False
    for t in range(STEPS):
        if events and t == T_PLACE:
            keys = place_events(orc.state, cap, last)
            if eng is not None:
                eng.upload_state({k: orc.state[k] for k in keys})
        before = orc.state["shape"]["flags"].reshape(E, cap).copy()
        resetting = orc.state["need_reset"].reshape(E) != 0
        a = actions(t)
        if eng is not None:
            eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        if eng is not None:
            assert_state_equal(eng.download_state(), orc.state, where="cap %d step %d" % (cap, t))
        after = orc.state["shape"]["flags"].reshape(E, cap)
        drove.append(drives(before) & ~resetting[:, None])
        if events and t == T_PLACE:
            removed = bool(drives(before[ENV_REMOVE:ENV_REMOVE + 1, last])[0] and not (after[ENV_REMOVE, last] & abi.F_ALIVE))
            reset_seen = bool(resetting[ENV_RESET]) and not resetting[ENV_REMOVE]
    return np.asarray(drove), removed, reset_seen


def check_cap_64_family(cap, step_engine=True):
    drove, removed, reset_seen = rollout(cap, targets=(cap - 1, 40), wake=3, cone_slot=50, events=True, step_engine=step_engine)
    assert not drove[T_PLACE, ENV_RESET].any(), "a resetting env drives nothing in that step"
    steps = drove.copy()
    steps[T_PLACE, ENV_RESET] = True                   # ... so it is left out of what follows
    assert steps[:T_PLACE, :, cap - 1].all(), "the last slot's vehicle must drive in every env"
    assert steps[:, :, 40].all(), "slot 40's vehicle must drive in every step of every env"
    assert steps[:, :, 0].all(), "the agents must drive"
    assert removed, "the step must remove the last slot's vehicle of env %d" % ENV_REMOVE
    assert reset_seen, "env %d must reset in the step of the removal" % ENV_RESET
    assert not drove[T_PLACE + 1:, ENV_REMOVE, cap - 1].any(), "the removed vehicle stays removed"
    assert drove[T_PLACE + 1:, ENV_RESET, cap - 1].all(), "the reset env drives its last slot again"


def test_cap_64_last_slot_drives_is_removed_and_an_env_resets():
    """the narrow kernel at its bound: mask bit 63, a slot >= 32, a prop between them"""
    check_cap_64_family(64)


@pytest.mark.parametrize("cap", [65, 72])
def test_caps_above_the_bound_keep_the_lean_kernel(cap):
    """the same scenes one and eight slots above the bound (the last slot is then 64 / 71: the masks' second word)"""
    check_cap_64_family(cap)


def check_small(cap, wake, step_engine=True):
    targets = (cap - 1, )
    drove, _, _ = rollout(cap, targets=targets, wake=wake, cone_slot=None, events=False, step_engine=step_engine)
    counts = drove.sum(axis=2)
    assert (counts[:3] >= wake + 1).all(), "%d traffic vehicles and the agent must drive from the start: %r" % (wake, counts[:3].tolist())
    assert drove[:, :, cap - 1].all()
    return counts


def test_cap_16_the_smallest_auto_size():
    check_small(16, 1)


def test_cap_24_four_traffic_vehicles_drive():
    """five and more driving vehicles: the localisations go in pairs, the IDM's rank walk deals four vehicles to three waves"""
    counts = check_small(24, 4)
    assert counts.min() >= 5
