"""The traffic trigger of the lean step kernel in two halves (csrc/parts/trigger.inc: trigger_search_wave beside the integration,
trigger_fire_wave in the traffic stage).  The search reads the waiting slots at the start of the step, the fire the agent's lane
after localisation; together they must clear exactly the blocks the oracle's trigger clears, bit for bit:
  rollouts: md_step against OracleWorld.step with fires, resets and several pending orders (and with none at all),
  placed states: one md_step from states where the fire must happen, must not happen, or the search's second chunk decides."""
import math

import numpy as np
import pytest

from helpers import assert_state_equal

pytestmark = pytest.mark.gpu

E = 8
SLOT = 0     # the agent's slot
DEFAULT = dict(start_seed=100, traffic_density=0.3, auto_reset=True, horizon=220)


def _engine_and_oracle(**kw):
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    import oracle_binding as ob
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    eng = BatchedEngine(make_config(dict(dict(num_envs=E, num_scenarios=E), **kw)))
    return eng, ob.OracleWorld(eng.host)


def _lane_follow_actions(orc, eng, t, random_envs=()):
    """Steer the agents along their current lane (they cross road boundaries); `random_envs` act at random and leave the road"""
    cap = eng.cap
    a = np.zeros((E, 1, 2), np.float32)
    env_map = eng.host.world.arrays["env_map"]
    rng = np.random.RandomState(977 + t)
    for e in range(E):
        n = e * cap + SLOT
        if e in random_envs:
            a[e, 0] = rng.uniform(-1, 1, 2)
            a[e, 0, 1] = abs(a[e, 0, 1])
            continue
        sh, l = orc.state["shape"][n], int(orc.state["nav"]["lane"][n])
        steer = 0.0
        if l >= 0:
            lane = eng.host.map_tables[int(env_map[e])].lane_objs[l]
            s, lat = lane.local_coordinates((float(sh["cx"]), float(sh["cy"])))
            err = math.atan2(float(sh["s"]), float(sh["c"])) - lane.heading_theta_at(min(max(s, 0.0), lane.length))
            err = (err + math.pi) % (2 * math.pi) - math.pi
            # lat > 0: right of the centre line, so steer left (positive); heading error the same way
            steer = max(-1.0, min(1.0, 0.3 * lat + 1.5 * err))
        a[e, 0] = (steer, 0.6 if float(orc.state["dyn"]["speed"][n]) < 12.0 else 0.0)
    return a


def _pending(shape_flags, cap):
    """[E, cap] bool: the slots the trigger's search sees (PENDING and ALIVE)"""
    from metadrive_ped_amd import abi
    f = shape_flags.reshape(E, cap)
    return ((f & abi.F_PENDING) != 0) & ((f & abi.F_ALIVE) != 0)


def _pending_orders(pend, nav, cap):
    """Per env: the set of distinct trigger orders among the pending slots"""
    order = nav["trigger_order"].reshape(E, cap)
    return [set(order[e][pend[e]].tolist()) for e in range(E)]


def _fired(before_pending, state, cap):
    """[E] bool: a slot the search saw lost its PENDING bit in this step (the removal clears ALIVE only, and never on such a slot)"""
    from metadrive_ped_amd import abi
    still = (state["shape"]["flags"].reshape(E, cap) & abi.F_PENDING) != 0
    return (before_pending & ~still).any(axis=1)


def _rollout(steps, **kw):
    """md_step against the oracle, all envs lane-following, states compared every step.
    -> (engine, fires per env, resets, env-steps with >= 2 pending orders, env-steps with nothing pending)"""
    import torch
    eng, orc = _engine_and_oracle(**kw)
    cap = eng.cap
    eng.reset()
    orc.reset()
    assert_state_equal(eng.download_state(), orc.state, where="reset")
    fires = np.zeros(E, np.int64)
    resets = multi = empty = 0
    for t in range(steps):
        a = _lane_follow_actions(orc, eng, t)
        # what the step's search sees: the live state, or the snapshot in an env that resets in this step
        resetting = orc.state["need_reset"].reshape(E) != 0
        seen = np.where(resetting[:, None], _pending(orc.state["shape0"]["flags"], cap), _pending(orc.state["shape"]["flags"], cap))
        live, snap = _pending_orders(seen, orc.state["nav"], cap), _pending_orders(seen, orc.state["nav0"], cap)
        for e in range(E):
            orders = snap[e] if resetting[e] else live[e]
            multi += len(orders) >= 2
            empty += len(orders) == 0
        resets += int(resetting.sum())
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        fires += _fired(seen, orc.state, cap)
        assert_state_equal(eng.download_state(), orc.state, where="step %d" % t)
    print("fires per env", fires.tolist(), "resets", resets, "env-steps with >= 2 pending orders", multi, "with none", empty)
    return eng, fires, resets, multi, empty


def test_rollout_default_distribution():
    """300 steps: every env fires several times and resets; the search almost always has two or more orders to choose from"""
    eng, fires, resets, multi, _ = _rollout(300, **DEFAULT)
    assert eng.host.step_kernel == "wg" and eng.w.max_lanes > 64, "the batch must take the lean, non-staged workgroup kernel"
    assert (fires >= 2).all(), fires
    assert resets >= 8, resets
    assert multi >= 1000, multi


def test_rollout_wider_capacity():
    """cap 72: the search's loops take a second 64-slot chunk"""
    eng, fires, resets, _, _ = _rollout(200, **dict(DEFAULT, mover_capacity=72, horizon=150))
    assert eng.cap == 72
    assert eng.host.step_kernel == "wg" and eng.w.max_lanes > 64
    assert (fires >= 1).all(), fires
    assert resets >= 4, resets


def test_rollout_no_traffic():
    """Nothing is ever pending: the search's empty result, and a fire that must do nothing"""
    steps = 60
    eng, fires, _, _, empty = _rollout(steps, **dict(DEFAULT, traffic_density=0.0, horizon=50))
    assert eng.host.step_kernel == "wg"
    assert (fires == 0).all(), fires
    assert empty == E * steps, empty


# ---- placed states -----------------------------------------------------------------------------------------------------------

PER_SLOT = ("shape", "dyn", "nav", "pid", "action", "flags", "param", "final_lane", "route_roads", "route_nodes")


class _PlacedBatch:
    """The default-distribution batch without auto-reset, a few steps in; `base` is the state every case starts from"""
    def __init__(self, **kw):
        import torch
        self.eng, self.orc = _engine_and_oracle(**dict(dict(DEFAULT, auto_reset=False), **kw))
        eng, orc = self.eng, self.orc
        assert eng.host.step_kernel == "wg" and eng.w.max_lanes > 64
        eng.reset()
        orc.reset()
        for t in range(3):
            a = _lane_follow_actions(orc, eng, t)
            eng.step(torch.from_numpy(a).to(eng.device))
            orc.step(a)
        assert_state_equal(eng.download_state(), orc.state, where="placed: start")
        self.cap = eng.cap
        self.base = {k: v.copy() for k, v in orc.state.items()}
        self.env_map = eng.host.world.arrays["env_map"]

    def restore(self):
        for k, v in self.base.items():
            self.orc.state[k][...] = v

    def tables(self, e):
        return self.eng.host.map_tables[int(self.env_map[e])]

    def trigger_roads(self, e):
        """[(order, trigger road)] of env e's pending blocks, lowest order first (the road of the lowest slot, as the search picks it)"""
        pend = _pending(self.base["shape"]["flags"], self.cap)[e]
        nav = self.base["nav"][e * self.cap:(e + 1) * self.cap]
        out = {}
        for j in np.nonzero(pend)[0]:
            out.setdefault(int(nav["trigger_order"][j]), int(nav["trigger_road"][j]))
        return sorted(out.items())

    def put_agent_on_road(self, e, road):
        """The agent of env e in the middle of the first lane of `road`, heading along it, that lane as its previous lane"""
        mt = self.tables(e)
        l = int(mt.roads["first_lane"][road])
        lane = mt.lane_objs[l]
        s = 0.5 * lane.length
        xy, th = lane.position(s, 0.0), lane.heading_theta_at(s)
        st, n = self.orc.state, e * self.cap + SLOT
        st["shape"]["cx"][n], st["shape"]["cy"][n] = np.float32(xy[0]), np.float32(xy[1])
        st["shape"]["c"][n], st["shape"]["s"][n] = np.float32(math.cos(th)), np.float32(math.sin(th))
        st["dyn"]["heading"][n], st["dyn"]["speed"][n] = np.float32(th), np.float32(0.0)
        st["nav"]["lane"][n] = l

    def step_both(self, where, need_reset=False):
        """One md_step against one orc.step from the oracle's present state -> the pending sets before the step"""
        import torch
        eng, orc = self.eng, self.orc
        orc.state["need_reset"][...] = 1 if need_reset else 0
        eng.upload_state(orc.state)
        assert_state_equal(eng.download_state(), orc.state, where=where + ": upload")
        seen = _pending(orc.state["shape0" if need_reset else "shape"]["flags"], self.cap)
        a = np.zeros((E, 1, 2), np.float32)
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        assert_state_equal(eng.download_state(), orc.state, where=where)
        return seen


@pytest.fixture(scope="module")
def placed():
    return _PlacedBatch()


def test_placed_agent_on_lowest_trigger_road(placed):
    """(a) the agent on a lane of the lowest pending block's trigger road: that block, and only that one, wakes"""
    placed.restore()
    lowest = {}
    for e in range(E):
        tr = placed.trigger_roads(e)
        assert tr, "env %d has nothing pending" % e
        lowest[e] = tr[0]
        placed.put_agent_on_road(e, tr[0][1])
    seen = placed.step_both("placed (a)")
    fired = _fired(seen, placed.orc.state, placed.cap)
    assert fired.any(), "the oracle cleared no block"
    after = _pending_orders(_pending(placed.orc.state["shape"]["flags"], placed.cap), placed.orc.state["nav"], placed.cap)
    for e in np.nonzero(fired)[0]:
        assert lowest[e][0] not in after[e]


def test_placed_agent_on_later_trigger_road(placed):
    """(b) the agent on the trigger road of a later block: the lowest order is not on that road, nothing wakes"""
    placed.restore()
    skipped = 0
    for e in range(E):
        tr = placed.trigger_roads(e)
        later = [road for _, road in tr[1:] if road != tr[0][1]]
        if not later:
            skipped += 1
            continue
        placed.put_agent_on_road(e, later[0])
    assert skipped <= E // 2, skipped
    seen = placed.step_both("placed (b)")
    assert not _fired(seen, placed.orc.state, placed.cap).any()


def test_placed_agent_off_every_lane(placed):
    """(c) the agent far from every lane, without a previous lane: the fire finds no agent lane"""
    placed.restore()
    st = placed.orc.state
    for e in range(E):
        n = e * placed.cap + SLOT
        st["shape"]["cx"][n] += np.float32(3000.0)
        st["shape"]["cy"][n] -= np.float32(2000.0)
        st["nav"]["lane"][n] = -1
    seen = placed.step_both("placed (c)")
    rows = np.arange(E) * placed.cap + SLOT
    assert (st["nav"]["lane"][rows] < 0).all()
    assert not _fired(seen, st, placed.cap).any()


def test_placed_reset_discards_placement(placed):
    """(e) case (a) with need_reset set: the step re-stages the snapshot, the search and the fire see the reset state"""
    placed.restore()
    for e in range(E):
        placed.put_agent_on_road(e, placed.trigger_roads(e)[0][1])
    placed.step_both("placed (e)", need_reset=True)
    assert not placed.orc.state["need_reset"].any()


def test_placed_second_chunk_decides():
    """(d) cap 72: a lowest-order pending slot moved to slot 70, so that the search's second 64-slot chunk holds the minimum"""
    from metadrive_ped_amd import abi
    b = _PlacedBatch(mover_capacity=72)
    cap = b.cap
    assert cap == 72
    st = b.orc.state
    moved = {}
    for e in range(E):
        tr = b.trigger_roads(e)
        assert tr, "env %d has nothing pending" % e
        order, road = tr[0]
        pend = _pending(b.base["shape"]["flags"], cap)[e]
        orders = b.base["nav"]["trigger_order"][e * cap:(e + 1) * cap]
        src = [int(j) for j in np.nonzero(pend & (orders == order))[0]]
        assert src and max(src) < 64, src
        assert not (b.base["shape"]["flags"][e * cap + 70] & abi.F_ALIVE), "slot 70 is taken"
        # every slot of that block in the first chunk is taken out, one of them lives on in slot 70
        for k in PER_SLOT:
            if k in st:
                rows = st[k].reshape(E * cap, -1)
                rows[e * cap + 70] = rows[e * cap + src[0]]
        for j in src:
            st["shape"]["flags"][e * cap + j] &= ~abi.F_ALIVE
        moved[e] = order
        b.put_agent_on_road(e, road)
    seen = b.step_both("placed (d)")
    for e in range(E):   # the lowest order is pending in slot 70 and nowhere in the first chunk
        first = b.base["nav"]["trigger_order"][e * cap:e * cap + 64]
        assert seen[e, 70] and not (seen[e, :64] & (first <= moved[e])).any()
    fl70 = st["shape"]["flags"].reshape(E, cap)[:, 70]
    fired = (fl70 & abi.F_PENDING) == 0
    assert fired.any(), "the oracle did not fire the moved slot"
