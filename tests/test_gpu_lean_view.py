"""The lean non-staged workgroup kernels derive an env's pointers where they are used, from the kernel-argument segment
(csrc/parts/lean_view.inc; the offsets are pinned by tests/test_kernarg_layout.py, which needs no GPU).  md_step against
OracleWorld.step on 6 envs over 60 steps, the whole state compared after every step; what each case is there for is asserted from
the oracle's states:
  resets at the horizon (the snapshots through pointers derived under do_reset), at capacity 24 (the narrow form) and 72 (its sibling),
  triggered traffic and a removed vehicle (the dirty-slot write-back through pointers derived behind the last barrier),
  MdState.agent_action absent (the null test the stage-in keeps),
  one staged-map batch: the kernel that keeps md_env_view, the control."""
import numpy as np
import pytest

from helpers import assert_state_equal, scripted_actions
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

E = 6
STEPS = 60
# start_seed 150: found on the CPU (the oracle alone) as the first of 100, 150, ... whose 60 steps trigger traffic AND remove a vehicle
TRAFFIC = dict(start_seed=150, traffic_density=0.3, auto_reset=True, horizon=1000)
RESETS = dict(start_seed=100, traffic_density=0.1, auto_reset=True, horizon=12)


def _pair(**kw):
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    import oracle_binding as ob
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    eng = BatchedEngine(make_config(dict(dict(num_envs=E, num_scenarios=E), **kw)))
    lean = eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and not eng.k.is_multi_agent and "detected" not in eng.state_dev
    assert lean and eng.host.step_kernel == "wg" and eng.k.agents_per_env == 1, "the batch must take a lean workgroup kernel"
    return eng, ob.OracleWorld(eng.host)


def _actions(t):
    a = scripted_actions(E, 1, t, seed=3)
    a[:, :, 0] *= 0.2
    return a


def _drives(flags):
    return ((flags & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((flags & abi.F_ALIVE) != 0) & ((flags & (abi.F_STATIC | abi.F_PENDING)) == 0)


def _rollout(eng, orc, step=None):
    """-> (resets per env, traffic slots triggered, driving traffic vehicles removed), counted on the oracle's states"""
    import torch
    cap = eng.cap
    eng.reset()
    orc.reset()
    assert_state_equal(eng.download_state(), orc.state, where="start")
    resets, triggered, removed = np.zeros(E, np.int64), 0, 0
    for t in range(STEPS):
        a = _actions(t)
        before = orc.state["shape"]["flags"].reshape(E, cap).copy()
        resetting = orc.state["need_reset"].reshape(E) != 0
        resets += resetting
        if step is None:
            eng.step(torch.from_numpy(a).to(eng.device))
        else:
            step(eng, a)
        orc.step(a)
        assert_state_equal(eng.download_state(), orc.state, where="step %d" % t)
        after = orc.state["shape"]["flags"].reshape(E, cap)
        live = ~resetting[:, None]
        waiting = ((before & abi.F_PENDING) != 0) & ((before & abi.F_ALIVE) != 0)
        triggered += int((waiting & ((after & abi.F_PENDING) == 0) & live)[:, 1:].sum())
        removed += int((_drives(before) & ((after & abi.F_ALIVE) == 0) & live)[:, 1:].sum())
    return resets, triggered, removed


@pytest.mark.parametrize("cap", [24, 72])
def test_every_env_resets_from_its_snapshot(cap):
    """capacity 24: the narrow form (at most 64 slots); 72: the lean kernel outside the size pins"""
    eng, orc = _pair(**dict(RESETS, mover_capacity=cap))
    assert eng.cap == cap and eng.w.max_lanes > 64, "the batch must take the non-staged kernel at this capacity"
    resets, _, _ = _rollout(eng, orc)
    assert (resets >= 1).all(), resets


def test_traffic_is_triggered_and_a_vehicle_removed():
    eng, orc = _pair(**TRAFFIC)
    assert eng.w.max_lanes > 64 and eng.cap <= 64
    _, triggered, removed = _rollout(eng, orc)
    assert triggered >= 1, "no traffic block was triggered"
    assert removed >= 1, "no driving vehicle was removed: the write-back of a slot marked kRemovedMark did not run"


def test_agent_action_absent():
    """MdState.agent_action null: the stage-in takes the agents' actions from the per-slot array"""
    eng, orc = _pair(**RESETS)
    assert eng.w.max_lanes > 64

    def step(eng, a):
        act = np.ascontiguousarray(eng.download_state()["action"])
        act.reshape(E, eng.cap, 2)[:, 0, :] = a[:, 0, :]
        eng.upload_state({"action": act})
        eng.s.agent_action = None
        eng.step_raw()

    resets, _, _ = _rollout(eng, orc, step=step)
    assert (resets >= 1).all(), resets


def test_staged_map_batch_is_unchanged():
    """map="S": the staged-map lean kernel, which still makes its view with md_env_view"""
    eng, orc = _pair(**dict(RESETS, map="S"))
    assert eng.w.max_lanes <= 64, "the batch must take the staged workgroup kernel"
    resets, _, _ = _rollout(eng, orc)
    assert (resets >= 1).all(), resets
