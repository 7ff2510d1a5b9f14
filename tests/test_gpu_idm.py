"""The device's IDM (csrc/parts/idm.inc: idm_candidates_wave and the three forms of the front / back scan -- idm_scan_wave, the pair
form; idm_scan_wave_keys, the key form; idm_scan_walks, beyond 21 candidates) on PLACED states.  After every launch
  (a) the whole downloaded state equals the oracle bit for bit;
  (b) for every decided driving vehicle nav.target_lane, nav.timer, nav.rand_cursor and pid.target_speed equal the float64
      reference of tests/idm_ref.py and the two action words lie within TOL_STEER / TOL_ACC of it.
The launch sets and their cases are idm_ref.IDM_RUNS / STEP_RUNS, the ones tests/test_idm_ref.py runs through the oracle alone.
Before any launch each test asserts from host data that the run takes the path it is named after, that every family its set must
hold is there, and that every named case sits where its name says (idm_ref.check_about on the env as placed)."""
import numpy as np
import pytest

import idm_ref as ir
from helpers import assert_state_equal
from metadrive_ped_amd import abi
from test_gpu_contacts import E, MAX_ROUNDS, Rig, _pg_engine, _rounds

pytestmark = pytest.mark.gpu

STAGE_MAX_LANES = 64      # kStageMaxLanes of csrc/mdstep.hip: up to here md_idm stages the map in LDS and scans in the pair form


class IdmRig:
    """the contact tests' rig (engine + oracle, the base state, one case per env) with what the IDM cases need on top: the idm_rand
    rows, a base without traffic, the map's float64 reference, the nav templates and the case builder"""
    def __init__(self, seq, cap=128, rest=False, **cfg):
        import ctypes as C
        self.rig = rig = Rig(_pg_engine(map=seq, mover_capacity=cap, **cfg))
        self.eng, self.orc, self.cap = rig.eng, rig.orc, rig.cap
        host = rig.eng.host
        assert rig.cap == cap and host.A == 1 and all(m is rig.mts[0] for m in rig.mts)
        self.mt = rig.mts[0]
        mt2, self.tmpl = ir.templates(seq)
        assert np.array_equal(mt2.lanes, self.mt.lanes) and np.array_equal(mt2.roads, self.mt.roads), "the harvest ran on another map"
        self.mr = ir.MapRef(self.mt, host.md_config.enable_idm_lane_change)
        self.idm_rand = ir.idm_rand_table(cap)
        rig.orc.state["idm_rand"].reshape(E, cap, abi.MD_IDM_RAND)[:] = self.idm_rand
        rig.eng.upload_state({"idm_rand": rig.orc.state["idm_rand"]})
        rig.base["idm_rand"] = rig.orc.state["idm_rand"].copy()
        ir.clear_traffic(rig.base, cap)
        self.builder = ir.Builder(self.mr, self.tmpl, rig.me0(), cap=cap, rest=rest, base_env=ir.env_rows(rig.base, 0, cap))
        self.tally = ir.Tally()
        lanes, lib = self.mt.lanes, rig.orc.lib

        def long_of(l, x, y):
            out = np.zeros(2, np.float32)
            lib.ref_lane_local(lanes[l:l + 1].ctypes.data, C.c_float(x), C.c_float(y), out.ctypes.data)
            return float(out[0])
        self.long_of = long_of

    def run(self, name, cases, launch, after_step):
        """place E cases at a time, assert their premises on the env as placed, launch on both sides, check (a) and (b)"""
        need = set(ir.NEEDED[name])
        assert need <= ir.families_of(cases), (name, sorted(need - ir.families_of(cases)))
        rounds = _rounds(cases)
        assert len(cases) <= MAX_ROUNDS * E
        for r, per_env in enumerate(rounds):
            self.rig.place(per_env, ir.PLACE_KEYS)
            placed = {k: self.orc.state[k].copy() for k in ("shape", "dyn", "nav", "pid")}
            for e, case in enumerate(per_env):
                ir.check_about(self.mr, ir.env_rows(placed, e, self.cap), case, self.idm_rand)
            launch()
            self.tally.launches += 1
            where = "%s round %d" % (name, r)
            got = self.eng.download_state()
            try:
                assert_state_equal(got, self.orc.state, where=where)
            except AssertionError as err:
                # which case it is: the float64 check names the env's case and the slot if it objects too, else the round's cases are listed
                for e, case in enumerate(per_env):
                    ir.check_env(self.mr, placed, got, e, self.cap, case, self.idm_rand, ir.Tally(), where, after_step=after_step)
                raise AssertionError("%s\n  (rows are env * %d + slot) envs of this round: %s" % (
                    err, self.cap, ", ".join("%d %s" % (e, c.name) for e, c in enumerate(per_env))))
            for e, case in enumerate(per_env):
                ir.check_env(self.mr, placed, got, e, self.cap, case, self.idm_rand, self.tally, where, after_step=after_step)
        self.tally.finish(name)
        assert need <= self.tally.families and self.tally.vehicles >= len(cases) and self.tally.moved == 0, (name, sorted(need - self.tally.families))


@pytest.mark.parametrize("name,seq,staged,curves", ir.IDM_RUNS, ids=[r[0] for r in ir.IDM_RUNS])
def test_md_idm_equals_oracle_and_float64_on_placed_states(name, seq, staged, curves):
    """md_idm alone against ref_idm.  A staged map (at most 64 lanes) scans in the pair form, any other in the key form; both enter
    the walks beyond 21 candidates (count_22, count_23, count_70 are in every set).  The `merge` set is the map with a road that
    loses lanes (forced_change)"""
    ctx = IdmRig(seq)
    n_lanes = int(ctx.eng.w.max_lanes)
    assert n_lanes == len(ctx.mt.lanes) and (n_lanes <= STAGE_MAX_LANES) == staged, (name, n_lanes)
    assert set(ir.WALK_FAMILIES) <= set(ir.NEEDED[name])
    cases = ir.idm_run_cases(ctx.builder, ctx.long_of, curves)

    def launch():
        ctx.eng.call("md_idm")
        ctx.orc.call("ref_idm")
    ctx.run(name, cases, launch, after_step=False)


@pytest.mark.parametrize("name,cfg,cap", ir.STEP_RUNS, ids=[r[0] for r in ir.STEP_RUNS])
def test_md_step_from_rest_plans_the_traffic(name, cfg, cap):
    """One md_step from rest with a zero agent action on a map of more than 64 lanes: the lean workgroup kernel (key form), its
    narrow form (one agent, at most 64 slots: the slot-64, slot-127 and count_70 cases are left out there, capacity 64 has no such
    slot), the one-wave-per-env kernel (idm_group_wave: the group family puts four driving vehicles into one env) and the respawn
    variant.  The step plans the traffic one step AHEAD: its IDM reads what the step's localiser left.  (a) in full.  (b) for every
    placed vehicle that still drives where it was placed, with the reference reading what the IDM does not write from the
    downloaded state (idm_ref.check_env); the rest of the step leaves nav.target_lane, nav.timer, nav.rand_cursor and
    pid.target_speed of such a vehicle alone, so all four are compared as well as the action words."""
    import torch
    ctx = IdmRig(ir.STEP_MAP, cap=cap, rest=True, **cfg)
    eng = ctx.eng
    lean = eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and "detected" not in eng.state_dev
    assert eng.host.step_kernel == cfg.get("step_kernel", "wg") and lean == (name != "respawn")
    assert int(eng.w.max_lanes) > STAGE_MAX_LANES and (eng.cap <= 64) == (name == "narrow") and eng.host.A == 1
    cases = ir.step_run_cases(ctx.builder, ctx.long_of)
    assert any(len(ir.driving_slots(ctx.builder.env_of(c))) >= 3 for c in cases if c.family == "group")
    zero = np.zeros((E, 1, 2), np.float32)

    def launch():
        eng.step(torch.from_numpy(zero).to(eng.device))
        ctx.orc.step(zero)
    ctx.run(name, cases, launch, after_step=True)
