"""The lean step kernel's locate stage with the agent's contacts as one flat pass over the quads of the up to four grid cells under
the chassis (csrc/parts/contacts.inc: contacts_vehicle<true>, include/md_geom.h: md_flat_cell_item) behind the mover loop.  md_step on PLACED
states of 8 envs on one 3-block map, mover capacity 8 and 24, against the oracle bit for bit (the whole state: flags, obs, reward,
cost, step_info, and the done words), placed as tests/test_gpu_contacts.py places them.  The cases are named after the grid cells
under the chassis and what lies in them; each runs with 1, 2, 3 and 5 driving vehicles in its env (two waves of the locate stage
without an item; one, which evaluates the observation ahead; the round full; localisations in pairs).  Every class is asserted from
the host tables and the placed state before the launch.  A rollout with an auto-reset in its middle follows."""
import math

import numpy as np
import pytest

import contact_ref as cr
import test_gpu_contacts as tc
from helpers import assert_state_equal
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

E = tc.E
K_WAVES = 4                       # waves of the step kernel's workgroup (MD_ENV_BLOCK / 64)
DRIVING = (1, 2, 3, 5)
OUTPUTS = ("flags", "obs", "reward", "cost", "done_out", "step_info")
# one map for all envs (seed chosen for: more than 64 lanes, so the batch takes the lean non-staged kernel; four and more parked
# traffic vehicles at both capacities; a cell without items; a pose over three kinds of quads)
RIGS = {8: dict(traffic_density=0.05, mover_capacity=8), 24: dict(traffic_density=0.1, mover_capacity=24)}
SEED = 5006
CONT = abi.FL_ON_WHITE_CONT | abi.FL_ON_YELLOW_CONT


def config(cap, **kw):
    return dict(dict(num_envs=E, num_scenarios=1, start_seed=SEED, auto_reset=False, **RIGS[cap]), **kw)


def _box(mt, pose):
    """the cell box under ONE chassis record -> (columns, rows), (0, 0) when the chassis is clear of the grid"""
    walked, gx0, gx1, gy0, gy1 = cr.cull_range(mt.grid, pose)
    return (int(gx1[0] - gx0[0]) + 1, int(gy1[0] - gy0[0]) + 1) if walked[0] else (0, 0)


def _quad_bits(mt, quads):
    bits = 0
    for q in quads:
        bits |= cr._QUAD_FLAG.get(int(mt.quad_kind[q]), 0)
    return bits


def _bits_by_cell(mt, pose, touched):
    """per walked cell: the flag bits of the touched quads that cell lists"""
    t = set(touched)
    return [_quad_bits(mt, [q for q, _ in cr.cell_quads(mt, c) if q in t]) for c in cr.walked_cells(mt, pose)]


def geometry_cases(mt, me0, rng):
    """-> {name: Case} for the named cell boxes, from the host tables alone"""
    poses, _ = cr.table_poses(mt, rng, n_random=600, every=max(1, len(mt.quads) // 60), n_border=900)
    want = {"one_cell": (1, 1), "vertical_edge": (2, 1), "horizontal_edge": (1, 2), "corner": (2, 2)}
    out, three = {}, None
    for i in rng.permutation(len(poses)):
        pose = poses[i:i + 1]
        box = _box(mt, pose)
        touched, decided = tc._touched(mt, pose)
        if not decided or not touched:
            continue
        bits = _quad_bits(mt, touched)
        for name, b in want.items():
            # a touched quad in every cell of the box for the edge / corner cases is not asked: one somewhere is
            if name not in out and box == b:
                out[name] = tc.Case(name, tc._posed(me0, pose[0]), [], (0x1F0, bits))
        per_cell = _bits_by_cell(mt, pose, touched)
        if three is None and (bits & CONT) and (bits & abi.FL_ON_BROKEN) and (bits & abi.FL_CRASH_SIDEWALK) and \
                len(per_cell) >= 2 and not any(b == bits for b in per_cell):
            three = tc.Case("three_kinds", tc._posed(me0, pose[0]), [], (0x1F0, bits))
        if len(out) == len(want) and three is not None:
            break
    assert set(out) == set(want), "no decided pose with a touched quad for the boxes %r" % sorted(set(want) - set(out))
    assert three is not None, "no pose over a continuous line, a broken line and a sidewalk with the bits from different cells"
    out["three_kinds"] = three
    empty = [c for c in tc._empty_cases(mt, me0) if c.name == "empty_cell"]
    assert empty, "the map has no cell without items that a chassis fits into"
    out["empty_cell"] = empty[0]
    edge, sides = tc._grid_edge_cases(mt, me0)
    assert sides, "no walked border cell lists a quad"
    out["border"] = edge
    return out


def vehicle_and_line(case, rng):
    """the agent of `case` (over a line) with a parked traffic vehicle across its chassis too: mover and quad bits in one step"""
    assert case.want[1] & 0x1F0
    body = tc._against(case.agent, "vehicle", -0.3, rng, flags=abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_PENDING)
    return tc.Case("vehicle_and_line", case.agent, [("free", body)], (cr.CONTACT_BITS, case.want[1] | abi.FL_CRASH_VEHICLE))


def parked(base_shape, cap):
    """env 0's parked traffic (PENDING vehicles) in the reset state -> their slots"""
    f = base_shape["flags"][:cap]
    return [int(j) for j in np.nonzero(((f & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((f & abi.F_ALIVE) != 0) & ((f & abi.F_PENDING) != 0) &
                                       ((f & (abi.F_AGENT | abi.F_STATIC)) == 0))[0]]


def free_slot(base_shape, cap):
    f = base_shape["flags"][:cap]
    free = np.nonzero(((f & abi.F_ALIVE) == 0) & ((f & abi.KIND_MASK) == abi.KIND_NONE))[0]
    assert len(free), "no free slot for the placed vehicle"
    return int(free[-1])


def with_driving(case, base_shape, cap, k):
    """`case` with k - 1 of the env's parked traffic vehicles awake (PENDING cleared, where they stand)"""
    bodies = [(free_slot(base_shape, cap) if s == "free" else s, r) for s, r in case.bodies]
    far = [j for j in parked(base_shape, cap)
           if math.hypot(float(base_shape[j]["cx"] - case.agent["cx"]), float(base_shape[j]["cy"] - case.agent["cy"])) > 8.0]
    assert len(far) >= k - 1, "case %s: fewer than %d parked vehicles stand clear of the agent" % (case.name, k - 1)
    for j in far[:k - 1]:
        rec = base_shape[j].copy()
        rec["flags"] = int(rec["flags"]) & ~abi.F_PENDING
        bodies.append((j, rec))
    return tc.Case(case.name, case.agent, bodies, case.want)


def drives(flags):
    return ((flags & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((flags & abi.F_ALIVE) != 0) & ((flags & (abi.F_STATIC | abi.F_PENDING)) == 0)


def rounds_of(mt, me0, base_shape, cap, seed=31):
    """-> [(k, [Case] * E)]: per driving count one round, the eight named cases one per env (the border case walks the grid's four
    sides over the rounds)"""
    rng = np.random.RandomState(seed)
    g = geometry_cases(mt, me0, rng)
    assert len(parked(base_shape, cap)) >= max(DRIVING) - 1, "the map parks fewer than %d vehicles" % (max(DRIVING) - 1)
    out = []
    for r, k in enumerate(DRIVING):
        named = [g["one_cell"], g["vertical_edge"], g["horizontal_edge"], g["corner"], g["border"][r % len(g["border"])], g["empty_cell"],
                 g["three_kinds"], vehicle_and_line(g["three_kinds"], rng)]
        assert len(named) == E
        out.append((k, [with_driving(c, base_shape, cap, k) for c in named]))
    return out


BOXES = {"one_cell": 1, "vertical_edge": 2, "horizontal_edge": 2, "corner": 4, "empty_cell": 1}


def assert_classes(mt, cap, k, per_env, placed_flags):
    """from the grid header and the placed state, before the launch: each case's cell box is the one it is named after and its env
    has k driving vehicles, the agent among them -> the classes (cells, schedule) of this round"""
    seen = set()
    for e, case in enumerate(per_env):
        pose = np.asarray([case.agent])
        cols, rows = _box(mt, pose)
        n_cells = cols * rows
        if case.name in BOXES:
            assert n_cells == BOXES[case.name], "case %s walks %d cells" % (case.name, n_cells)
        if case.name == "vertical_edge":
            assert (cols, rows) == (2, 1)
        if case.name == "horizontal_edge":
            assert (cols, rows) == (1, 2)
        if case.name == "empty_cell":
            assert all(not cr.cell_quads(mt, c) for c in cr.walked_cells(mt, pose))
        if case.name.startswith("grid_edge"):
            gx0, gx1, gy0, gy1 = tc._unclamped(mt, pose)
            gr = mt.grid[0]
            assert gx0 < 0 or gy0 < 0 or gx1 >= int(gr["nx"]) or gy1 >= int(gr["ny"]), "case %s: no cell index is clamped" % case.name
            seen.add("clamped")
        assert 1 <= n_cells <= 4
        seen.add("%d cells" % n_cells)
        d = drives(placed_flags[e * cap:(e + 1) * cap])
        nd, na = int(d.sum()), int(d[0])
        assert (nd, na) == (k, 1), "case %s env %d: %d driving vehicles, agent driving %d; wanted %d" % (case.name, e, nd, na, k)
        seen.add("one round, two free waves" if nd + na + 1 < K_WAVES else "one round, a free wave" if nd + na < K_WAVES else
                 "one round, full" if nd + na == K_WAVES else "localisations in pairs")
    return seen


@pytest.mark.parametrize("cap", sorted(RIGS))
def test_md_step_on_placed_states_by_cells_and_driving_vehicles(cap):
    import torch

    def make():
        from metadrive_ped_amd.config import make_config
        from metadrive_ped_amd.engine import BatchedEngine
        return BatchedEngine(make_config(config(cap)))
    rig = tc.Rig(make)
    eng, orc = rig.eng, rig.orc
    lean = eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and "detected" not in eng.state_dev
    assert lean and eng.host.step_kernel == "wg" and eng.w.max_lanes > 64 and rig.cap == cap, "the batch must take the lean, non-staged workgroup kernel"
    mt, me0 = rig.mts[0], rig.me0()
    assert all(m is mt for m in rig.mts)
    keys = ("shape", "dyn", "flags", "nav", "route_roads")
    zero = np.zeros((E, 1, 2), np.float32)
    seen = set()
    for k, per_env in rounds_of(mt, me0, rig.base["shape"], cap):
        rig.place(per_env, keys)
        placed = orc.state["shape"].copy()
        seen |= assert_classes(mt, cap, k, per_env, placed["flags"])
        eng.step(torch.from_numpy(zero).to(eng.device))
        orc.step(zero)
        where = "cap %d, %d driving" % (cap, k)
        assert_state_equal(eng.download_state(), orc.state, keys=OUTPUTS, where=where)
        rig.check(per_env, where)
        now = orc.state["shape"]
        assert np.array_equal(now["cx"][::cap], placed["cx"][::cap]) and np.array_equal(now["cy"][::cap], placed["cy"][::cap]), \
            "the step moved an agent at rest: its cells are not the placed ones"
    rig.finish("locate contacts, cap %d" % cap)
    need = {"1 cells", "2 cells", "4 cells", "clamped", "one round, two free waves", "one round, a free wave", "one round, full", "localisations in pairs"}
    assert need <= seen, "classes that never occurred: %r" % sorted(need - seen)
    bits = abi.FL_CRASH_VEHICLE | abi.FL_ON_BROKEN | abi.FL_CRASH_SIDEWALK
    assert (rig.seen & bits) == bits and (rig.seen & CONT), "flags never raised; seen %#x" % rig.seen


def test_rollout_with_an_auto_reset_in_its_middle():
    """60 steps of horizon 30 on eight maps with traffic, the agents following their lanes (the actions of
    tests/test_gpu_observe_lockstep.py), so that blocks trigger and one to five and more vehicles drive: every env resets at step
    30; the whole state after every step"""
    import torch
    import oracle_binding as ob
    from test_gpu_observe_lockstep import _actions
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    eng = BatchedEngine(make_config(dict(num_envs=E, num_scenarios=E, start_seed=5000, traffic_density=0.1, mover_capacity=24, auto_reset=True, horizon=30)))
    assert eng.host.step_kernel == "wg" and eng.w.max_lanes > 64, "the batch must take the lean, non-staged workgroup kernel"
    orc = ob.OracleWorld(eng.host)
    eng.reset()
    orc.reset()
    resets, counts = set(), set()
    for t in range(60):
        a = _actions(orc, eng.host, t)
        if (orc.state["need_reset"].reshape(E) != 0).any():
            resets.add(t)
        counts |= set(drives(orc.state["shape"]["flags"].reshape(E, eng.cap)).sum(1).tolist())
        eng.step(torch.from_numpy(a).to(eng.device))
        orc.step(a)
        got = eng.download_state()
        assert_state_equal(got, orc.state, keys=OUTPUTS, where="step %d" % t)
        assert_state_equal(got, orc.state, where="step %d (whole state)" % t)
    assert resets and 20 <= min(resets) and max(resets) <= 40, "no reset step in the middle of the rollout: %r" % sorted(resets)
    assert {1, 2, 3} <= counts and max(counts) >= 5, "driving vehicles per env over the rollout: %r" % sorted(counts)
