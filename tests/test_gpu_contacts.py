"""The device's contact walk (contacts_vehicle, csrc/parts/contacts.inc) on PLACED states: the grid cull under the chassis AABB, the
64-strided cell loop, the two 64-wide mover chunks, the nine-ballot OR and the flag merge of the lean step kernels.  After every
launch the whole state equals the oracle bit for bit, and bits 0x1FF of every agent's flag word equal the float64 reference of
tests/contact_ref.py wherever that is decided, evaluated on the downloaded shapes.  Each named case asserts from the host tables,
before the launch, that it still exercises the path it is named after."""
import math

import numpy as np
import pytest

import contact_ref as cr
from helpers import assert_state_equal
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

E = 8
MAX_ROUNDS = 40
ALIVE = abi.F_ALIVE
# kind -> (hl, hw, shape flags of a body the step does not move, the flag it raises)
BODIES = {"vehicle": (2.2, 0.9, abi.KIND_VEHICLE | ALIVE | abi.F_STATIC, abi.FL_CRASH_VEHICLE),
          "cone": (0.2, 0.2, abi.KIND_CONE | ALIVE | abi.F_STATIC, abi.FL_CRASH_OBJECT),
          "warning": (0.25, 0.25, abi.KIND_WARNING | ALIVE | abi.F_STATIC, abi.FL_CRASH_OBJECT),
          "barrier": (0.15, 1.0, abi.KIND_BARRIER | ALIVE | abi.F_STATIC, abi.FL_CRASH_OBJECT),
          "pedestrian": (0.35, 0.35, abi.KIND_PEDESTRIAN | ALIVE, abi.FL_CRASH_HUMAN),
          "cyclist": (0.875, 0.2, abi.KIND_CYCLIST | ALIVE, abi.FL_CRASH_HUMAN),
          "building": (5.0, 5.0, abi.KIND_BUILDING | ALIVE | abi.F_STATIC, abi.FL_CRASH_BUILDING)}
MOVER_BITS = 0xF


class Case:
    """One placed env: the agent's pose (None: where the reset left it), bodies [(slot, record)], and for a named case the bits
    (mask, value) its flag word must show"""
    def __init__(self, name, agent=None, bodies=(), want=None):
        self.name, self.agent, self.bodies, self.want = name, agent, list(bodies), want


def _body(kind, ctr, th, flags=None, hl=None, hw=None):
    bl, bw, fl, _ = BODIES[kind]
    r = cr.make_shapes([ctr[0]], [ctr[1]], np.asarray([th]), bl if hl is None else hl, bw if hw is None else hw, fl if flags is None else flags)
    r["aux"] = -1
    return r[0]


def _against(me, kind, gap, rng, flags=None, axis=None, frac=None, hl=None, hw=None):
    """a body of `kind` whose nearest corner (a circle: its rim) lies `gap` metres off a face of the chassis record `me`"""
    bl, bw = BODIES[kind][0] if hl is None else hl, BODIES[kind][1] if hw is None else hw
    th = math.atan2(float(me["s"]), float(me["c"]))
    axis = np.asarray([rng.randint(0, 2) if axis is None else axis])
    sign = np.asarray([1.0 if rng.randint(0, 2) else -1.0])
    frac = np.asarray([rng.uniform(-0.8, 0.8) if frac is None else frac])
    ctr = np.asarray([[float(me["cx"]), float(me["cy"])]])
    p, n = cr.face_point(ctr, np.asarray([th]), np.asarray([float(me["hl"])]), np.asarray([float(me["hw"])]), axis, sign, frac)
    bth = th + (0.0, 0.5 * math.pi, rng.uniform(-math.pi, math.pi))[rng.randint(0, 3)]
    if (BODIES[kind][2] & abi.KIND_MASK) in cr.CIRCLE_KINDS:
        c = p + n * (bl + gap)
    else:
        c = cr.centre_with_corner_at(p + n * gap, n, np.asarray([bth]), np.asarray([bl]), np.asarray([bw]))
    return _body(kind, c[0], bth, flags, hl, hw)


def _posed(me0, pose):
    me = me0.copy()
    for k in ("cx", "cy", "c", "s"):
        me[k] = pose[k]
    return me


def _mover_cases(me, rng, with_pending):
    """the named cases about the mover loop, around the chassis record `me` (clear of every other body)"""
    hit = lambda kind, **kw: _against(me, kind, -0.3, rng, **kw)
    out = [Case("self", me, [], (MOVER_BITS, 0)),
           Case("last_lane_63", me, [(63, hit("vehicle"))], (MOVER_BITS, abi.FL_CRASH_VEHICLE)),
           Case("second_chunk_64", me, [(64, hit("vehicle"))], (MOVER_BITS, abi.FL_CRASH_VEHICLE)),
           Case("second_chunk_127", me, [(127, hit("cone"))], (MOVER_BITS, abi.FL_CRASH_OBJECT)),
           Case("not_alive", me, [(9, hit("vehicle", flags=abi.KIND_VEHICLE | abi.F_STATIC))], (MOVER_BITS, 0)),
           Case("kind_none", me, [(70, hit("vehicle", flags=abi.KIND_NONE | ALIVE))], (MOVER_BITS, 0)),
           # a circle kind's radius is hl: hw = 3 m must not reach the chassis from 0.5 m, hl = 0.6 m must
           Case("circle_ignores_hw", me, [(3, _against(me, "cone", 0.3, rng, hl=0.2, hw=3.0))], (MOVER_BITS, 0)),
           Case("circle_radius_is_hl", me, [(3, _against(me, "cone", -0.1, rng, hl=0.6, hw=0.01))], (MOVER_BITS, abi.FL_CRASH_OBJECT))]
    for i, (kind, (_, _, _, flag)) in enumerate(sorted(BODIES.items())):
        out.append(Case("one_" + kind, me, [(5 + 17 * i, hit(kind))], (MOVER_BITS, flag)))
        out.append(Case("near_" + kind, me, [(6 + 17 * i, _against(me, kind, 0.05, rng))], (MOVER_BITS, 0)))
    if with_pending:     # parked traffic of a block that is not triggered yet has a body
        out.append(Case("pending", me, [(64, hit("vehicle", flags=abi.KIND_VEHICLE | ALIVE | abi.F_PENDING))], (MOVER_BITS, abi.FL_CRASH_VEHICLE)))
    return out


def _scatter(me, rng, with_pending):
    """a few bodies of random kinds around the chassis, touching and not, in slots of both 64-wide chunks"""
    slots = rng.permutation(np.r_[1:8, 60:68, 120:128])[:rng.randint(0, 6)]
    kinds = sorted(BODIES)
    out = []
    for s in slots:
        kind = kinds[rng.randint(0, len(kinds))]
        flags = None
        if kind == "vehicle" and with_pending and rng.randint(0, 2):
            flags = abi.KIND_VEHICLE | ALIVE | abi.F_PENDING
        out.append((int(s), _against(me, kind, (0.01, -0.01, 0.3, -0.3, 2.0)[rng.randint(0, 5)], rng, flags=flags)))
    return out


def _unclamped(mt, pose):
    f = np.float32
    g = mt.grid[0]
    c, s, hl, hw = (pose[k].astype(f) for k in ("c", "s", "hl", "hw"))
    ex, ey = np.abs(c) * hl + np.abs(s) * hw + f(0.05), np.abs(s) * hl + np.abs(c) * hw + f(0.05)
    lo = lambda v, e, o: int(np.floor((v.astype(f) - e - f(o)) * f(g["inv_cell"]))[0])
    hi = lambda v, e, o: int(np.floor((v.astype(f) + e - f(o)) * f(g["inv_cell"]))[0])
    return lo(pose["cx"], ex, g["x0"]), hi(pose["cx"], ex, g["x0"]), lo(pose["cy"], ey, g["y0"]), hi(pose["cy"], ey, g["y0"])


def _touched(mt, pose):
    """quads the float64 reference says the chassis touches, decidedly"""
    cand = cr.candidate_quads(mt, pose)
    if not len(cand):
        return [], True
    hit, decided = cr.obb_quad(np.repeat(pose, len(cand)), mt.quads[cand])
    return [int(q) for q in cand[hit]], bool(decided.all())


def _two_cells_case(mt, me0, rng):
    """a chassis whose walk visits two cells, the touched quads listed in the second only"""
    for q in rng.permutation(len(mt.quads)):
        for i in range(4):
            th = rng.uniform(-math.pi, math.pi)
            pose = cr.agent_poses(cr.approach_edge(mt.quads[q], i, 0.5, -0.02, th)[None], th)
            cells = cr.walked_cells(mt, pose)
            touched, decided = _touched(mt, pose)
            if len(cells) != 2 or not touched or not decided:
                continue
            first, second = (set(k for k, _ in cr.cell_quads(mt, c)) for c in cells)
            if not (set(touched) & first) and set(touched) <= second:
                bits = 0
                for k in touched:
                    bits |= cr._QUAD_FLAG[int(mt.quad_kind[k])]
                return Case("two_cells", _posed(me0, pose[0]), [], (0x1F0, bits))
    raise AssertionError("no pose walks two cells with its quads in the second only")


def _grid_edge_cases(mt, me0):
    """the chassis half outside the grid on each of its four sides, next to the quad that reaches farthest that way -> (cases, the
    sides on which a walked cell lists a quad)"""
    g = mt.grid[0]
    cell = 1.0 / float(g["inv_cell"])
    x0, y0, x1, y1 = float(g["x0"]), float(g["y0"]), float(g["x0"]) + int(g["nx"]) * cell, float(g["y0"]) + int(g["ny"]) * cell
    v = mt.quads.astype(np.float64).reshape(-1, 2)
    out, sides = [], set()
    for side, ctr in (("west", (x0, v[v[:, 0].argmin(), 1])), ("east", (x1, v[v[:, 0].argmax(), 1])),
                      ("south", (v[v[:, 1].argmin(), 0], y0)), ("north", (v[v[:, 1].argmax(), 0], y1))):
        pose = cr.agent_poses(np.asarray([ctr]), 0.0 if side in ("west", "east") else 0.5 * math.pi)
        gx0, gx1, gy0, gy1 = _unclamped(mt, pose)
        beyond = {"west": gx0 < 0, "east": gx1 >= int(g["nx"]), "south": gy0 < 0, "north": gy1 >= int(g["ny"])}[side]
        cells = cr.walked_cells(mt, pose)
        assert beyond and cells, (side, ctr, (gx0, gx1, gy0, gy1))
        if any(cr.cell_quads(mt, c) for c in cells):
            sides.add(side)
        out.append(Case("grid_edge_" + side, _posed(me0, pose[0])))
    return out, sides


def _empty_cases(mt, me0):
    """clear of everything: outside the grid, and in the middle of a cell that lists nothing"""
    g = mt.grid[0]
    cell = 1.0 / float(g["inv_cell"])
    out = [Case("empty_outside", _posed(me0, cr.agent_poses(np.asarray([[float(g["x0"]) - 30.0, float(g["y0"]) - 30.0]]), 0.7)[0]), [],
                (cr.CONTACT_BITS, 0))]
    bare = np.nonzero(np.diff(mt.cell_start) == 0)[0]
    if len(bare):
        c = int(bare[0])
        ctr = [[float(g["x0"]) + (c % int(g["nx"]) + 0.5) * cell, float(g["y0"]) + (c // int(g["nx"]) + 0.5) * cell]]
        pose = cr.agent_poses(np.asarray(ctr), 0.3)
        if cr.walked_cells(mt, pose) == [c]:
            out.append(Case("empty_cell", _posed(me0, pose[0]), [], (cr.CONTACT_BITS, 0)))
    return out


def _clear_of_bodies(rig, mt, me0):
    """where the mover cases stand: the agent's own spawn pose, or -- with traffic around it -- a pose beside the grid"""
    own = rig.base["shape"][1:rig.cap]
    near = ((own["flags"] & ALIVE) != 0) & (np.hypot(own["cx"] - me0["cx"], own["cy"] - me0["cy"]) <= 15.0)
    if not near.any():
        return me0
    g = mt.grid[0]
    return _posed(me0, cr.agent_poses(np.asarray([[float(g["x0"]) - 30.0, float(g["y0"]) - 30.0]]), 0.7)[0])


def _table_cases(mt, me0, rng, n, with_pending):
    poses, tag = cr.table_poses(mt, rng, n_random=n // 3, every=max(1, 8 * len(mt.quads) // max(1, n // 3)), n_border=n // 3)
    pick = rng.permutation(len(poses))[:n]
    out = []
    for p in pick:
        me = _posed(me0, poses[p])
        out.append(Case(str(tag[p]), me, _scatter(me, rng, with_pending)))
    return out


class Rig:
    """engine + oracle on one config, reset, with the state the reset left as the base every placement starts from"""
    def __init__(self, make, retag=False, tracks=False):
        import torch
        import oracle_binding as ob
        assert torch.cuda.is_available(), "GPU tests need a ROCm device"
        self.torch = torch
        self.eng = eng = make()
        host = eng.host
        a = host.world.arrays
        self.mts = [host.map_tables[int(m)] for m in a["env_map"]]
        if retag:      # no table builder emits crosswalks: every fourth quad becomes one, on the host, on the device, then in the oracle
            kinds = a["quad_kind"]
            kinds[::4] = abi.Q_CROSSWALK
            eng.world_dev["quad_kind"].copy_(torch.from_numpy(kinds.view(np.uint8).reshape(-1)))
            for m, mt in enumerate(host.map_tables):
                mt.quad_kind = kinds[a["quad_off"][m]:a["quad_off"][m + 1]].copy()
        for m, mt in enumerate(host.map_tables):
            lo, hi = int(a["quad_off"][m]), int(a["quad_off"][m + 1])
            assert np.array_equal(a["quads"].reshape(-1, 8)[lo:hi], mt.quads) and np.array_equal(a["quad_kind"][lo:hi], mt.quad_kind)
        self.orc = orc = ob.OracleWorld(host)
        if tracks:
            orc.set_tracks(host.tracks["shape"], host.tracks["dyn"])
        eng.reset()
        orc.reset()
        self.cap = eng.cap
        self.base = {k: v.copy() for k, v in orc.state.items()}
        assert_state_equal(eng.download_state(), self.base, where="reset")
        self.cases = self.undecided = self.seen = 0
        self.rounds = 0

    def me0(self, e=0, slot=0):
        me = self.base["shape"][e * self.cap + slot].copy()
        assert me["flags"] & abi.F_AGENT and abs(float(me["hl"]) - cr.AGENT_HL) < 1e-6 and abs(float(me["hw"]) - cr.AGENT_HW) < 1e-6
        return me

    def place(self, per_env, keys):
        """write one Case per env into the oracle's state (restored from the base first) and upload it"""
        st = self.orc.state
        for k in keys:
            st[k][...] = self.base[k]
        for e, case in enumerate(per_env):
            rows = st["shape"][e * self.cap:(e + 1) * self.cap]
            for slot, rec in [(0, case.agent)] * (case.agent is not None) + case.bodies:
                assert 0 <= slot < self.cap and np.isfinite([rec["cx"], rec["cy"], rec["c"], rec["s"]]).all()
                assert math.hypot(float(rec["cx"]), float(rec["cy"])) < 2000.0, "poses stay within 2 km of the origin"
                rows[slot] = rec
                if "dyn" in keys:      # at rest, heading as placed
                    d = st["dyn"][e * self.cap + slot]
                    d["heading"], d["speed"] = math.atan2(float(rec["s"]), float(rec["c"])), 0.0
                    d["last_x"], d["last_y"], d["last_c"], d["last_s"] = rec["cx"], rec["cy"], rec["c"], rec["s"]
                    st["dyn"][e * self.cap + slot] = d
            for k, rows in getattr(case, "rows", {}).items():      # whole records of other state arrays (tests/idm_ref.py: dyn, nav, pid)
                assert k in keys
                for slot, rec in rows:
                    st[k][e * self.cap + slot] = rec
        self.eng.upload_state({k: st[k] for k in keys})

    def check(self, per_env, where, agent_slots=(0, )):
        """after the launch on both sides: bit parity of the whole state, then the flag words against float64"""
        assert self.rounds < MAX_ROUNDS
        self.rounds += 1
        got = self.eng.download_state()
        assert_state_equal(got, self.orc.state, where=where)
        words = []
        for e, case in enumerate(per_env):
            shp = got["shape"][e * self.cap:(e + 1) * self.cap]
            for slot in agent_slots:
                want, decided = cr.agent_flags(shp, slot, self.mts[e].quads, self.mts[e].quad_kind)
                g = int(got["flags"][e * self.cap + slot]) & cr.CONTACT_BITS
                words.append(g)
                f = int(shp["flags"][slot])
                if not (f & ALIVE and f & abi.F_AGENT and (f & abi.KIND_MASK) == abi.KIND_VEHICLE) or f & (abi.F_STATIC | abi.F_PENDING):
                    continue       # not a driving agent: the contact stage leaves its word alone
                assert ((g ^ want) & decided) == 0, "%s env %d (%s) slot %d: device %#x, float64 %#x, decided bits %#x; agent %s" % (
                    where, e, case.name, slot, g, want, decided, shp[slot].tolist())
                self.cases += 1
                self.undecided += decided != cr.CONTACT_BITS
                self.seen |= g
            if case.want is not None:
                g = int(got["flags"][e * self.cap]) & cr.CONTACT_BITS
                assert (g & case.want[0]) == case.want[1], "%s env %d: case %s shows %#x, must show %#x under mask %#x" % (
                    where, e, case.name, g, case.want[1], case.want[0])
        return words

    def finish(self, name):
        print("%s: %d rounds, %d agent poses, %d undecided, flags seen %#x" % (name, self.rounds, self.cases, self.undecided, self.seen))
        assert self.undecided <= cr.UNDECIDED_CAP * self.cases, (name, self.undecided, self.cases)


def _pg_engine(**kw):
    def make():
        from metadrive_ped_amd.config import make_config
        from metadrive_ped_amd.engine import BatchedEngine
        return BatchedEngine(make_config(dict(dict(num_envs=E, num_scenarios=1, traffic_density=0.0, mover_capacity=128, auto_reset=False), **kw)))
    return make


def _rounds(cases):
    """the cases dealt over the envs: round r places cases[r * E + e] in env e (the last round is filled up from the first)"""
    cases = cases[:MAX_ROUNDS * E]
    cases = cases + cases[:(-len(cases)) % E]
    return [cases[r * E:(r + 1) * E] for r in range(len(cases) // E)]


def _assert_premises(rig, per_env):
    """what the named cases are named after, from the host tables, before the launch"""
    for e, case in enumerate(per_env):
        present = [s for s, r in case.bodies if (int(r["flags"]) & ALIVE) and (int(r["flags"]) & abi.KIND_MASK)]
        if case.name in ("last_lane_63", "second_chunk_64", "second_chunk_127"):
            assert present == [int(case.name.rsplit("_", 1)[1])] and rig.cap == 128
        if case.want is not None and case.want[0] == MOVER_BITS:
            # nothing but the placed body is near: what the map itself put into the env (toll booths) stands far away
            own = rig.base["shape"][e * rig.cap + 1:(e + 1) * rig.cap]
            far = np.hypot(own["cx"] - case.agent["cx"], own["cy"] - case.agent["cy"]) > 15.0
            assert (far | ((own["flags"] & ALIVE) == 0)).all()
        if case.name == "self":
            assert not case.bodies
        if case.name.startswith("one_") or case.name in ("pending", "circle_radius_is_hl"):
            assert len(present) == 1


@pytest.mark.parametrize("name,seq", [("intersection", "X"), ("roundabout", "O"), ("curve", "C"), ("tollgate", "S$S")])
def test_md_contacts_equals_oracle_and_float64_on_placed_states(name, seq):
    """(a) md_contacts alone against ref_contacts; crosswalk quads retagged in"""
    rig = Rig(_pg_engine(map=seq), retag=True)
    mt, me0 = rig.mts[0], rig.me0()
    assert all(m is mt for m in rig.mts) and rig.cap == 128 and (mt.quad_kind == abi.Q_CROSSWALK).sum() > 20
    rng = np.random.RandomState(17)
    edge, sides = _grid_edge_cases(mt, me0)
    named = _mover_cases(me0, rng, True) + [_two_cells_case(mt, me0, rng)] + edge + _empty_cases(mt, me0)
    cases = named + _table_cases(mt, me0, rng, MAX_ROUNDS * E - len(named), True)
    assert {"self", "last_lane_63", "second_chunk_64", "second_chunk_127", "not_alive", "kind_none", "pending", "circle_ignores_hw",
            "circle_radius_is_hl", "two_cells", "empty_outside", "edge", "border", "random"} <= set(c.name for c in cases)
    assert sides == {"west", "east", "south", "north"}, "a walked border cell lists no quad on some side: %s" % sorted(sides)
    keys = ("shape", "flags")
    for r, per_env in enumerate(_rounds(cases)):
        _assert_premises(rig, per_env)
        rig.place(per_env, keys)
        rig.eng.call("md_contacts")
        rig.orc.call("ref_contacts")
        rig.check(per_env, "%s md_contacts round %d" % (name, r))
    rig.finish(name)
    need = MOVER_BITS
    for k in set(mt.quad_kind.tolist()):
        need |= cr._QUAD_FLAG[k]
    assert need & abi.FL_ON_CROSSWALK and (rig.seen & need) == need, "flags never raised: %#x" % (need & ~rig.seen)


# (respawn mode needs traffic to be a mode at all: without any the config falls back to the lean path's trigger mode)
STEP_RUNS = [("wg", dict(step_kernel="wg")), ("wave", dict(step_kernel="wave")),
             ("respawn", dict(traffic_mode="respawn", traffic_density=0.1))]


@pytest.mark.parametrize("name,extra", STEP_RUNS, ids=[n for n, _ in STEP_RUNS])
def test_md_step_from_rest_merges_the_contact_flags(name, extra):
    """(b) one md_step from rest with a zero action: the flag word the step kernels merge (the lean ones through their staged
    flag buffer, the respawn variant straight into the state) around obstacles the step does not move"""
    import torch
    rig = Rig(_pg_engine(map="X", **extra), retag=True)
    eng, orc = rig.eng, rig.orc
    lean = eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and "detected" not in eng.state_dev
    assert eng.host.step_kernel == extra.get("step_kernel", "wg") and lean == (name != "respawn")
    mt, me0 = rig.mts[0], rig.me0()
    rng = np.random.RandomState(23)
    named = _mover_cases(_clear_of_bodies(rig, mt, me0), rng, False) + [_two_cells_case(mt, me0, rng)] + _grid_edge_cases(mt, me0)[0] + _empty_cases(mt, me0)
    cases = named + _table_cases(mt, me0, rng, 20 * E - len(named), False)
    keys = ("shape", "dyn", "flags", "nav", "route_roads")
    zero = np.zeros((E, 1, 2), np.float32)
    for r, per_env in enumerate(_rounds(cases)):
        _assert_premises(rig, per_env)
        rig.place(per_env, keys)
        placed = orc.state["shape"].copy()
        eng.step(torch.from_numpy(zero).to(eng.device))
        orc.step(zero)
        rig.check(per_env, "%s md_step round %d" % (name, r))
        now = orc.state["shape"]
        rows = np.asarray([e * rig.cap + s for e, c in enumerate(per_env) for s in [0] + [s for s, _ in c.bodies]])
        assert np.array_equal(now["cx"][rows], placed["cx"][rows]) and np.array_equal(now["cy"][rows], placed["cy"][rows]), \
            "the step moved a body at rest"
        assert np.array_equal(now["flags"][rows], placed["flags"][rows])
    rig.finish(name)
    assert (rig.seen & 0x1FF) == 0x1FF, "flags never raised: %#x" % (0x1FF & ~rig.seen)


def test_multi_agent_contacts():
    """(c) a roundabout env of six agents: every agent's flag word; two agents across each other both crash, an agent over a dead
    slot does not"""
    A = 6

    def make():
        from metadrive_ped_amd.engine import BatchedEngine
        from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentRoundaboutEnv
        return BatchedEngine(BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, num_scenarios=E, num_agents=A, auto_reset=False)).config)
    rig = Rig(make)
    cap = rig.cap
    fl = rig.base["shape"]["flags"].reshape(E, cap)
    assert cap == A and ((fl & abi.F_AGENT) != 0).all() and ((fl & ALIVE) != 0).all()
    rng = np.random.RandomState(29)
    slots = tuple(range(A))
    for r in range(4):
        per_env = []
        for e in range(E):
            me = rig.me0(e, 0)
            across = rig.base["shape"][e * cap + 1].copy()
            across["cx"], across["cy"] = me["cx"], me["cy"]
            across["c"], across["s"] = -me["s"], me["c"]                    # the second agent lies across the first
            over = rig.base["shape"][e * cap + 2].copy()
            dead = rig.base["shape"][e * cap + 3].copy()
            dead["flags"] = int(dead["flags"]) & ~ALIVE
            dead["cx"], dead["cy"] = over["cx"], over["cy"]                 # the third agent stands over a dead slot
            shift = np.float32(rng.uniform(-0.5, 0.5))
            across["cx"] += shift
            per_env.append(Case("across", me, [(1, across), (2, over), (3, dead)]))
        rig.place(per_env, ("shape", "flags"))
        rig.eng.call("md_contacts")
        rig.orc.call("ref_contacts")
        words = np.asarray(rig.check(per_env, "marl round %d" % r, agent_slots=slots)).reshape(E, A)
        assert (words[:, 0] & abi.FL_CRASH_VEHICLE).all() and (words[:, 1] & abi.FL_CRASH_VEHICLE).all(), words
        assert ((words[:, 2] & MOVER_BITS) == 0).all(), words
    rig.finish("marl")


def test_scenario_step_strided_cell_walk():
    """(d) the scenario kernel on the dense scene of tests/test_contact_tables.py: cells that list more than 64 quads"""
    import torch
    from test_contact_tables import dense_scenario, dense_strided_pose

    def make():
        from metadrive_ped_amd.engine import BatchedEngine
        from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config
        cfg = make_scenario_config(dict(num_envs=E, num_scenarios=E, auto_reset=False))
        return BatchedEngine(cfg, host=ScenarioHostScene(cfg, [dense_scenario() for _ in range(E)]))
    rig = Rig(make, tracks=True)
    eng, orc, mt = rig.eng, rig.orc, rig.mts[0]
    me0 = rig.base["shape"][0].copy()
    assert me0["flags"] & abi.F_AGENT and np.diff(mt.cell_start).max() > 64
    strided, q = dense_strided_pose(mt, float(me0["hl"]), float(me0["hw"]))
    touched, decided = _touched(mt, strided)
    where = [dict(cr.cell_quads(mt, c)).get(q) for c in cr.walked_cells(mt, strided)]
    assert touched == [q] and decided and any(w is not None for w in where) and all(w is None or w >= 64 for w in where), (touched, where)
    rng = np.random.RandomState(37)
    band = cr.agent_poses(np.stack([rng.uniform(-35.0, 35.0, 5 * E), rng.uniform(-4.0, 16.0, 5 * E)], -1), rng.uniform(-math.pi, math.pi, 5 * E))
    cases = [Case("strided_cell", _posed(me0, strided[0]), [], (cr.CONTACT_BITS, abi.FL_ON_WHITE_CONT)),
             Case("clear", _posed(me0, cr.agent_poses(np.asarray([[0.0, -20.0]]), 0.4)[0]), [], (cr.CONTACT_BITS, 0))]
    cases += [Case("band", _posed(me0, band[i])) for i in range(len(band))]
    zero = np.zeros((E, 1, 2), np.float32)
    for r, per_env in enumerate(_rounds(cases)):
        rig.place(per_env, ("shape", "dyn", "flags"))
        eng.step(torch.from_numpy(zero).to(eng.device))
        orc.step(zero)
        rig.check(per_env, "scenario round %d" % r)
    rig.finish("scenario")
    assert rig.seen & abi.FL_ON_WHITE_CONT
