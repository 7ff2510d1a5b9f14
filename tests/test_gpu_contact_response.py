"""Contact response on the MI355X (md_contact_response, include/md_contact_response.h): the engine -- md_contact_response before
md_ped and md_step -- against the host rule (tests/contact_response_host.c) applied to the CPU oracle's state before each of its
steps, bit for bit in every state array and step output, in the step-kernel variants, with two lane rounds, in partly filled
workgroups, in a multi-agent env and beside the crossing pedestrians; the launch count; snapshots.  The runs are the ones at which
the host alone shows resolved contacts (tests/test_contact_response.py: PARITY_RUNS; found with the same host rollout)."""
import numpy as np
import pytest

import contact_response_host as ch
from helpers import assert_state_equal
from metadrive_ped_amd import abi
from test_contact_response import PARITY_RUNS, VARIANT_STEPS, VARIANTS, constant_actions, parity_user

pytestmark = pytest.mark.gpu


def _check(env, res, orc, where):
    st = env.engine.download_state()
    assert_state_equal(st, orc.state, keys=list(st), where=where)
    if res is not None:
        obs, reward, terminated, truncated, _ = res
        E, A = env.num_envs, env.engine.A
        assert obs.cpu().numpy().tobytes() == orc.state["obs"].tobytes(), where
        assert reward.cpu().numpy().tobytes() == orc.state["reward"].tobytes(), where
        done = orc.state["done_out"].reshape(E, A, 4)
        assert np.array_equal(terminated.cpu().numpy().reshape(E, A), done[..., 0] != 0), where
        assert np.array_equal(truncated.cpu().numpy().reshape(E, A), done[..., 1] != 0), where


def _parity(name, steps=None, ped=False, **extra):
    import metadrive_ped_amd.envs as envs
    user, n, cls = parity_user(name, **extra)
    env = getattr(envs, cls)(user)
    env.reset()
    eng = env.engine
    assert eng._cr is not None and abs(eng._cr.skin - 0.01) < 1e-9 and eng._cr.max_push == 0.5
    orc = ch.ContactOracle(eng.host, ped=abi.make_md_ped(eng.host.cfg["pedestrian_config"]) if ped else None)
    orc.reset()
    _check(env, None, orc, "reset")
    a = constant_actions(eng.E, eng.A)
    for t in range(steps or n):
        res = env.step(a[:, 0] if eng.A == 1 else a)
        orc.step(a)
        _check(env, res, orc, "%s step %d" % (name, t))
    return env, orc


def test_parity_single_agent():
    env, orc = _parity("single")
    assert env.engine.host.step_kernel == "wg" and env.engine.k.traffic_mode == 0 and env.engine.cap <= 64
    c = orc.cover
    assert c.vehicle_immovable >= 1 and c.vehicle_vehicle >= 1, (c.vehicle_immovable, c.vehicle_vehicle)
    assert (orc.resets >= 2).all(), orc.resets          # the reset of env.reset() and an auto-reset, in every env: none was skipped


def test_parity_multi_agent():
    env, orc = _parity("multi")
    assert env.engine.A == 12 and env.engine.k.is_multi_agent
    assert orc.cover.agent_agent >= 1


@pytest.mark.parametrize("name", [n for n in VARIANTS if n != "peds"])
def test_parity_variants(name):
    extra = VARIANTS[name]
    env, orc = _parity("single", steps=VARIANT_STEPS, **extra)
    eng = env.engine
    assert eng.host.step_kernel == extra.get("step_kernel", "wg")
    assert eng.cap == extra.get("mover_capacity", eng.cap) and eng.E == extra.get("num_envs", 8)
    assert eng.k.traffic_mode == (1 if "traffic_mode" in extra else 0)
    assert orc.cover.resolved >= 1, "the variant's run must hold a contact"


def test_parity_with_pedestrians_pins_the_launch_order():
    """The rule, then md_ped (tests/ped_host.c), then the step: a pedestrian judges the corrected vehicles"""
    import ped_host
    env, orc = _parity("single", steps=VARIANT_STEPS, ped=True, **VARIANTS["peds"])
    assert (ped_host.driven_slots(orc.state, 8, env.engine.cap).sum(axis=1) == 2).all()
    assert orc.cover.resolved >= 1


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("md_") or name == "md_last_error":
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


def _env(on, steps, **extra):
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    seed, cfg, _, _ = PARITY_RUNS["single"]
    env = BatchedMetaDriveEnv(dict(cfg, start_seed=seed, contact_response=on, **extra))
    env.reset()
    a = constant_actions(8, 1)
    for t in range(steps):
        env.step(a[:, 0])
    return env


def test_one_more_launch_per_step_in_front_of_everything():
    calls = {}
    for on in (False, True):
        env = _env(on, 2, num_pedestrians=2)
        assert (env.engine._cr is None) == (not on)
        lib = env.engine.lib = _CountingLib(env.engine.lib)
        env.step(constant_actions(8, 1)[:, 0])
        calls[on] = list(lib.calls)
    assert "md_contact_response" not in calls[False] and calls[False][:2] == ["md_ped", "md_step"] and calls[False].count("md_step") == 1
    assert calls[True] == ["md_contact_response"] + calls[False]


def test_off_by_default():
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=2, num_scenarios=2))
    env.reset()
    assert env.config["contact_response"] is False and env.engine._cr is None


def test_snapshot_and_restore_reproduce_the_run():
    env = _env(True, 60)
    snap = env.snapshot()
    a = constant_actions(8, 1)

    def run():
        out = []
        for t in range(50):                 # the host rollout's first contact falls on step 72
            res = env.step(a[:, 0])
            out.append(([x.cpu().numpy().copy() for x in res[:4]], env.engine.download_state()))
        return out

    first = run()
    env.restore(snap)
    again = run()
    for t, ((oa, sa), (ob_, sb)) in enumerate(zip(first, again)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(oa, ob_)), t
        assert_state_equal(sa, sb, keys=list(sa), where="after restore, step %d" % t)
    # the continuation held contacts: the rule was at work in it
    host = env.engine.host
    cover = ch.Coverage()
    for _, st in first:
        before = {k: st[k].copy() for k in ch.KEYS}
        after = {k: st[k].copy() for k in ch.KEYS}
        ch.apply(after, ch.config_struct(host.E, host.cap), ch.params())
        cover.note(before, after, host.E, host.cap)
    assert cover.resolved >= 1
