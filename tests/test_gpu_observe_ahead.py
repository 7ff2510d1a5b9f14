"""The lean step kernel with the agent's observation evaluated ahead (csrc/parts/observe.inc: observe_ahead_wave beside the localisation, the hit
path of observe_agent_wave1) against the oracle, which evaluates it after the localisation like every other kernel: md_step rollouts of
8 envs x 120 steps with auto_reset and horizon 60, every step's whole state bit for bit.  Traffic densities: none (every env has one driving
vehicle), 0.1, 0.3, and 0.8, at which most envs have three and more driving vehicles, so that no wave is left without an item.
What makes the kernel keep or drop the ahead results is read from the oracle's state before and after each step, and every such event
must occur in the rollouts (tests/test_observe_ahead.py shows the same on the oracle alone, without a GPU)."""
import pytest

from helpers import assert_state_equal
from test_gpu_observe_lockstep import E, SLOT, STEPS, OUTPUTS, _actions, _engine

K_WAVES = 4              # waves of the step kernel's workgroup (MD_ENV_BLOCK / 64)
KEY_FIELDS = ("lane", "road0", "road1", "ck0", "ck1")
BASE = dict(num_envs=E, num_scenarios=E, start_seed=5000, auto_reset=True, horizon=60)
# density 0.1 (the benchmark's) is there for the envs with TWO driving vehicles: at 0.3 a block's trigger wakes several at once, and
# these rollouts go from one driving vehicle to three and more
CONFIGS = {"no traffic": dict(BASE, traffic_density=0.0), "density 0.1": dict(BASE, traffic_density=0.1),
           "density 0.3": dict(BASE, traffic_density=0.3), "dense": dict(BASE, traffic_density=0.8)}
KEPT_1, KEPT_2, LANE_ALONE, CHECKPOINT, RESET, NO_FREE_WAVE = (
    "key kept with nd = 1", "key kept with nd = 2", "lane changed alone", "checkpoint advance", "reset step", "nd + na >= kWaves")
NEEDED = {"no traffic": {KEPT_1, LANE_ALONE, CHECKPOINT, RESET},
          "density 0.1": {KEPT_1, KEPT_2, LANE_ALONE, CHECKPOINT, RESET, NO_FREE_WAVE},
          "density 0.3": {KEPT_1, CHECKPOINT, RESET, NO_FREE_WAVE},
          "dense": {KEPT_1, NO_FREE_WAVE, RESET}}


def _drives(flags):
    from metadrive_ped_amd import abi
    return ((flags & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((flags & abi.F_ALIVE) != 0) & ((flags & (abi.F_STATIC | abi.F_PENDING)) == 0)


def _events(cap, before_flags, before_nav, after_nav, resetting):
    """The oracle's state before and after a step -> the set of event names.  The driving slots of a step are those of the state it
    starts from (the trigger of a step fires at the end of the one before); a resetting env starts from its snapshot instead."""
    out = set()
    if resetting.any():
        out.add(RESET)
    drv = _drives(before_flags.reshape(E, cap))
    for e in range(E):
        if resetting[e]:
            continue
        nd, na = int(drv[e].sum()), int(drv[e, SLOT])
        n = e * cap + SLOT
        same = {f: int(before_nav[f][n]) == int(after_nav[f][n]) for f in KEY_FIELDS}
        if nd + na >= K_WAVES:
            out.add(NO_FREE_WAVE)
            continue
        if na and all(same.values()) and nd in (1, 2):
            out.add(KEPT_1 if nd == 1 else KEPT_2)
        if not same["lane"] and all(same[f] for f in KEY_FIELDS[1:]):
            out.add(LANE_ALONE)
        if not same["ck0"] or not same["road0"]:
            out.add(CHECKPOINT)
    return out


def rollout(config, steps=STEPS, eng=None):
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
    seen = set()
    for t in range(steps):
        a = _actions(orc, host, t)
        resetting = orc.state["need_reset"].reshape(E) != 0
        before_flags, before_nav = orc.state["shape"]["flags"].copy(), orc.state["nav"].copy()
        orc.step(a)
        seen |= _events(host.cap, before_flags, before_nav, orc.state["nav"], resetting)
        if eng is not None:
            eng.step(torch.from_numpy(a).to(eng.device))
            got = eng.download_state()
            assert_state_equal(got, orc.state, keys=OUTPUTS, where="step %d" % t)
            assert_state_equal(got, orc.state, where="step %d (whole state)" % t)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_rollout_bit_exact_with_every_event(name):
    seen = rollout(CONFIGS[name], eng=_engine(CONFIGS[name]))
    assert NEEDED[name] <= seen, "%s: the rollout lacks %r" % (name, sorted(NEEDED[name] - seen))
