"""The float64 IDM reference of tests/idm_ref.py against the CPU oracle's ref_idm, CPU only -- where a wrong formula in the shared
headers (md_fb_neighbour, md_idm_policy, md_idm_act: compiled into the device and the oracle alike) surfaces:
  (a) on every case of every map that tests/test_gpu_idm.py launches, wherever the vehicle is decided, nav.target_lane, nav.timer,
      nav.rand_cursor and pid.target_speed are equal and the two action words lie within TOL_STEER / TOL_ACC; the six front / back
      buckets of every named ego equal the oracle's md_find_front_back;
  (b) MARGIN, TOL_STEER and TOL_ACC are the measured ones (printed), with their sanity conditions;
  (c) every named family sits where its name says, shows its bucket in the action (sensitivity), and is decided; the undecided
      share stays under its cap;
  (d) the reference is not trivially agreeable: permuting the slots of non-tied bodies leaves its result unchanged, shifting an
      object across a window flips it."""
import ctypes as C
import math

import numpy as np
import pytest

import idm_ref as ir
import oracle_binding as ob
from metadrive_ped_amd import abi

E = 8
MAX_LAUNCHES = 40


class CpuRig:
    """the oracle alone on one config, reset, with the state the reset left (its traffic taken out) as the base every placement
    starts from: the host-side twin of the device test's rig"""
    def __init__(self, seq, cap=128, rest=False, **kw):
        from metadrive_ped_amd.config import make_config
        from metadrive_ped_amd.engine import HostScene
        host = HostScene(make_config(dict(dict(num_envs=E, num_scenarios=1, traffic_density=0.0, mover_capacity=cap, auto_reset=False, map=seq), **kw)))
        self.host, self.cap = host, host.cap
        assert host.cap == cap and host.A == 1
        self.orc = ob.OracleWorld(host)
        self.orc.reset()
        self.mt = host.map_tables[0]
        assert all(int(m) == 0 for m in host.world.arrays["env_map"])
        mt2, self.tmpl = ir.templates(seq)
        assert np.array_equal(mt2.lanes, self.mt.lanes) and np.array_equal(mt2.roads, self.mt.roads), "the harvest ran on another map"
        self.mr = ir.MapRef(self.mt, host.md_config.enable_idm_lane_change)
        self.idm_rand = ir.idm_rand_table(self.cap)
        self.orc.state["idm_rand"].reshape(E, self.cap, abi.MD_IDM_RAND)[:] = self.idm_rand
        self.base = {k: v.copy() for k, v in self.orc.state.items()}
        ir.clear_traffic(self.base, self.cap)
        self.builder = ir.Builder(self.mr, self.tmpl, self.base["shape"][0].copy(), cap=self.cap, rest=rest, base_env=ir.env_rows(self.base, 0, self.cap))
        self.lib = self.orc.lib

    def lane_local(self, l, x, y):
        out = np.zeros(2, np.float32)
        self.lib.ref_lane_local(self.mt.lanes[l:l + 1].ctypes.data, C.c_float(x), C.c_float(y), out.ctypes.data)
        return out

    def long_of(self, l, x, y):
        return float(self.lane_local(l, x, y)[0])

    def oracle_buckets(self, env, slot, ids):
        """md_find_front_back of the oracle on one env's rows -> (front[3] + back[3], their distances)"""
        shapes, navs = np.ascontiguousarray(env["shape"]), np.ascontiguousarray(env["nav"])
        ids3 = np.asarray(ids, np.int32)
        out6, dist6 = np.zeros(6, np.int32), np.zeros(6, np.float32)
        self.lib.ref_front_back(self.mt.lanes.ctypes.data, shapes.ctypes.data, navs.ctypes.data, self.cap, slot, ids3.ctypes.data,
                                C.c_float(float(shapes["cx"][slot])), C.c_float(float(shapes["cy"][slot])), out6.ctypes.data, dist6.ctypes.data)
        return out6, dist6


_RUNS = {}


def run_of(name):
    """(rig, cases, after_step) of one launch set of idm_ref.IDM_RUNS / STEP_RUNS"""
    if name not in _RUNS:
        for n, seq, staged, curves in ir.IDM_RUNS:
            if n == name:
                rig = CpuRig(seq)
                assert (len(rig.mt.lanes) <= 64) == staged
                _RUNS[name] = (rig, ir.idm_run_cases(rig.builder, rig.long_of, curves), False)
        for n, cfg, cap in ir.STEP_RUNS:
            if n == name:
                rig = CpuRig(ir.STEP_MAP, cap=cap, rest=True, **cfg)
                _RUNS[name] = (rig, ir.step_run_cases(rig.builder, rig.long_of), True)
    return _RUNS[name]


ALL_RUNS = [r[0] for r in ir.IDM_RUNS] + [r[0] for r in ir.STEP_RUNS]


def run_oracle(rig, cases, tally, after_step, gaps=None, premises=False):
    """ref_idm (a whole ref_step from rest) over the cases, E at a time; every driving vehicle against the float64 reference.
    premises: every named case sits where its name says in the env as placed, and the oracle's own md_find_front_back fills the six
    buckets of its egos as the reference does -> the number of buckets compared"""
    st = rig.orc.state
    zero = np.zeros((E, 1, 2), np.float32)
    assert len(cases) <= MAX_LAUNCHES * E
    n_buckets = 0
    for r in range(0, len(cases), E):
        per_env = cases[r:r + E]
        ir.place_rows(st, rig.base, per_env, rig.cap, ir.PLACE_KEYS)
        placed = {k: st[k].copy() for k in ("shape", "dyn", "nav", "pid")}
        for e, case in enumerate(per_env if premises else ()):
            env = ir.env_rows(placed, e, rig.cap)
            for ego, res in ir.check_about(rig.mr, env, case, rig.idm_rand).items():
                if res.participant or res.plan["fail"]:
                    continue
                slots, dist = rig.oracle_buckets(env, ego, res.plan["ids"])
                for i in range(3):
                    for k, side in ((i, "front"), (3 + i, "back")):
                        assert int(slots[k]) == res.fb[side][i], (case.name, ego, i, side, slots.tolist(), res.fb)
                        assert abs(float(dist[k]) - res.fb[side + "_d"][i]) <= ir.MARGIN, (case.name, ego, i, side, dist.tolist(), res.fb)
                        n_buckets += 1
        if after_step:
            rig.orc.step(zero)
        else:
            rig.orc.call("ref_idm")
        tally.launches += 1
        for e, case in enumerate(per_env):
            ir.check_env(rig.mr, placed, st, e, rig.cap, case, rig.idm_rand, tally, "oracle", after_step=after_step, gaps=gaps)
    return n_buckets


@pytest.mark.parametrize("name", ALL_RUNS)
def test_oracle_equals_float64_on_placed_cases(name):
    """(a) and (c)"""
    rig, cases, after_step = run_of(name)
    fams = ir.families_of(cases)
    need = set(ir.NEEDED[name])
    assert need <= fams, (name, sorted(need - fams))
    print("%s: %d lanes, %d template lanes, %d cases; families %s" % (name, rig.mr.n, len(rig.tmpl), len(cases), " ".join(sorted(fams))))
    tally = ir.Tally()
    n_buckets = run_oracle(rig, cases, tally, after_step, premises=True)
    print("%s: %d buckets of named egos equal the oracle's" % (name, n_buckets))
    tally.finish(name)
    assert tally.vehicles >= len(cases) and tally.moved == 0 and need <= tally.families and n_buckets >= 6 * len(need)


def test_named_families_exist_somewhere():
    """a family that one map cannot offer (no axis-aligned lane, no straight predecessor, no road that loses lanes) runs on another"""
    fams = set()
    for name in [r[0] for r in ir.IDM_RUNS]:
        fams |= ir.families_of(run_of(name)[1])
    assert set(ir.ALL_FAMILIES) <= fams, sorted(set(ir.ALL_FAMILIES) - fams)


def test_constants_are_the_measured_ones():
    """(b) MARGIN: 4 x the largest gap between ref_lane_local and the float64 projection over every projection the cases need;
    TOL_STEER / TOL_ACC: 4 x the largest oracle-to-float64 gap of the action words over all decided vehicles"""
    worst_s = worst_lat = 0.0
    gaps = []
    for name in ALL_RUNS:
        rig, cases, after_step = run_of(name)
        rig.mr.log = []
        try:
            run_oracle(rig, cases, ir.Tally(), after_step, gaps=gaps)
        finally:
            log, rig.mr.log = rig.mr.log, None
        seen = set()
        m_s = m_lat = 0.0
        for l, x, y, s, lat in log:
            if (l, x, y) in seen:
                continue
            seen.add((l, x, y))
            got = rig.lane_local(l, x, y)
            m_s, m_lat = max(m_s, abs(float(got[0]) - s)), max(m_lat, abs(float(got[1]) - lat))
        print("%s: %d projections, largest |ref_lane_local - float64| longitudinal %.2e m, lateral %.2e m; lane graph margin %.3f m" % (
            name, len(seen), m_s, m_lat, rig.mr.graph_margin))
        worst_s, worst_lat = max(worst_s, m_s), max(worst_lat, m_lat)
        assert rig.mr.graph_margin > 100.0 * ir.MARGIN
    d_steer, d_acc = max(g[0] for g in gaps), max(g[1] for g in gaps)
    print("projections: longitudinal %.2e m, lateral %.2e m -> 4 x = %.2e m; MARGIN %.1e" % (worst_s, worst_lat, 4.0 * worst_s, ir.MARGIN))
    print("action words over %d decided vehicles: steering %.2e (%s), acceleration %.2e relative to max(1, |acc|) (%s) -> 4 x = %.2e, %.2e; "
          "TOL_STEER %.1e, TOL_ACC %.1e" % (len(gaps), d_steer, max(gaps, key=lambda g: g[0])[2], d_acc, max(gaps, key=lambda g: g[1])[2],
                                           4.0 * d_steer, 4.0 * d_acc, ir.TOL_STEER, ir.TOL_ACC))
    # the written constants: 4 x the measured gap, rounded UP to one digit -- and no more than that
    assert ir.MARGIN == _round_up(4.0 * worst_s) and ir.MARGIN < ir.MARGIN_CAP
    assert ir.TOL_STEER == _round_up(4.0 * d_steer) and ir.TOL_ACC == _round_up(4.0 * d_acc)
    assert ir.SENS_FACTOR == 100.0 and ir.UNDECIDED_CAP == 0.05


def _round_up(v):
    """to one significant digit of 1, 2 or 5"""
    e = 10.0 ** math.floor(math.log10(v))
    for m in (1.0, 2.0, 5.0, 10.0):
        if v <= m * e * (1.0 + 1e-12):
            return float("%.0e" % (m * e))


def test_permuting_slots_leaves_the_reference_unchanged():
    """(d) the slots of the bodies of the fill cases (no ties there) permuted: the same decision and action"""
    rig = run_of("nonstaged_intersection")[0]
    rng = np.random.RandomState(3)
    idm_rand = rig.idm_rand
    n = 0
    for case in ir.fill_cases(rig.builder, 30):
        env = rig.builder.env_of(case)
        a = ir.evaluate(rig.mr, env, ir.EGO, idm_rand[ir.EGO], sensitivity=False)
        slots = [s for s, _ in case.bodies if s != ir.EGO]
        if len(slots) < 2 or not a.decided:
            continue
        perm = dict(zip(slots, rng.permutation(slots)))
        env2 = {k: v.copy() for k, v in env.items()}
        for s, t in perm.items():
            for k in env:
                env2[k][t] = env[k][s]
        b = ir.evaluate(rig.mr, env2, ir.EGO, idm_rand[ir.EGO], sensitivity=False)
        assert (a.steering, a.acc, a.timer, a.target_speed, a.target_lane) == (b.steering, b.acc, b.timer, b.target_speed, b.target_lane), case.name
        for key in ("front", "back"):
            assert [perm.get(j, j) for j in a.fb[key]] == b.fb[key], (case.name, a.fb, b.fb)
        n += 1
    assert n >= 15


def test_shifting_an_object_across_a_window_flips_the_reference():
    """(d) the window family's pairs differ in the bucket and in the action"""
    rig = run_of("staged_straight")[0]
    idm_rand = rig.idm_rand
    res = {}
    for case in ir.window_cases(rig.builder):
        res[case.name.split(":")[1]] = ir.evaluate(rig.mr, rig.builder.env_of(case), ir.EGO, idm_rand[ir.EGO])
    for a, b in (("front_29.5", "front_30.5"), ("front_0.5", "front_-0.5")):
        assert res[a].fb["front"][1] == 5 and res[b].fb["front"][1] == -1
        assert abs(res[a].acc - res[b].acc) > ir.SENS_FACTOR * ir.acc_tol(res[a].acc)
    for a, b in (("back_29.5", "back_30.5"), ("back_0.5", "back_-0.5")):
        assert res[a].fb["back"][0] == 5 and res[b].fb["back"][0] == -1
    assert res["back_0.5"].policy["steer_lane"] != res["back_30.5"].policy["steer_lane"]
