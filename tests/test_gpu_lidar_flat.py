"""The lean non-staged workgroup kernels' lidar (lidar_agent_flat, csrc/mdstep.hip): one wave casts an agent's whole cloud, flat over
the (mover, beam) pairs inside the movers' beam spans (md_lidar_beam_span), minima taken in LDS.  On PLACED states, one md_step from
rest with a zero action, 4 envs: capacity 24 (the narrow kernel) and 72 (its sibling, the candidates in slots on both sides of 64),
fans of 240 beams (three full sectors and a part one) and of 30.  After the step the WHOLE state -- the cloud in obs with it --
equals the oracle's bit for bit; the oracle casts every beam at every mover.  Each case asserts on the ORACLE's own cloud that it
shows what it is named for; run(..., step_engine=False) runs the oracle alone, which is how the cases were chosen on the CPU."""
import math

import numpy as np
import pytest

import sensor_ref as sr
from helpers import assert_state_equal
from metadrive_ped_amd import abi

pytestmark = pytest.mark.gpu

E = 4
FAR = 600.0          # metres off every lane


def _slots(cap, n):
    """n free slots: at capacity 72 on both sides of slot 64"""
    lo = 1 if cap <= 64 else min(64 - n // 2, cap - n)
    assert lo + n <= cap
    return list(range(lo, lo + n))


def _case_none(ego, B, cap):
    o, u, ang = sr._beam(ego, B, B // 2)
    return ego, [(_slots(cap, 1)[0], sr.body("vehicle", o + u * 80.0, ang))]


def _case_absent(ego, B, cap):
    o, u, ang = sr._beam(ego, B, 1 % B)
    gone = ego.copy()
    gone["flags"] = int(ego["flags"]) & ~abi.F_ALIVE
    return gone, [(_slots(cap, 1)[0], sr.body("vehicle", o + u * 8.0, ang + 0.5 * math.pi))]


def _case_wrap(ego, B, cap):
    o, u, ang = sr._beam(ego, B, 0)
    return ego, [(_slots(cap, 2)[1], sr.body("vehicle", o + u * (12.0 if B >= 64 else 6.0), ang + 0.5 * math.pi))]


def _case_inside_circle(ego, B, cap):
    """inside a building's bounding circle (6 m < 7.07 m), a metre outside its box: every beam is a candidate"""
    o, u, ang = sr._beam(ego, B, B // 3)
    return ego, [(_slots(cap, 3)[2], sr.body("building", o + u * 6.0, ang, hl=5.0, hw=5.0))]


def _case_long_span(ego, B, cap):
    """just outside the circle: at 240 beams the span is longer than one pass of 64 lanes (one owner over two passes)"""
    o, u, ang = sr._beam(ego, B, (2 * B) // 3)
    return ego, [(_slots(cap, 4)[3], sr.body("building", o + u * 7.5, ang, hl=5.0, hw=5.0))]


def _case_many(ego, B, cap):
    """22 pedestrians on a ring of 3.5 m: at 240 beams more than 128 pairs, the owners change inside a pass and at pass boundaries"""
    o = np.array([float(ego["cx"]), float(ego["cy"])])
    return ego, [(s, sr.body("pedestrian", o + sr._unit(0.1 + 2.0 * math.pi * k / 22.0) * 3.5, 0.0)) for k, s in enumerate(_slots(cap, 22))]


def _case_tie(ego, B, cap):
    o, u, ang = sr._beam(ego, B, B // 5)
    rec = sr.body("vehicle", o + u * 9.0, ang + 0.5 * math.pi)
    s = _slots(cap, 12)
    return ego, [(s[11], rec), (s[2], rec.copy())]


def _case_removed(ego, B, cap):
    """agent and a DRIVING traffic vehicle ten metres ahead of it, both far off every lane: the traffic stage removes the vehicle
    in this step, so the lidar does not see it"""
    me = ego.copy()
    me["cx"], me["cy"] = float(ego["cx"]) + FAR, float(ego["cy"]) + FAR
    o, u, ang = sr._beam(me, B, 0)
    return me, [(_slots(cap, 6)[5], sr.body("vehicle", o + u * 10.0, ang + 0.5 * math.pi, flags=abi.KIND_VEHICLE | abi.F_ALIVE))]


CASES = [("none", _case_none), ("absent", _case_absent), ("wrap", _case_wrap), ("inside_circle", _case_inside_circle),
         ("long_span", _case_long_span), ("many", _case_many), ("tie", _case_tie), ("removed", _case_removed)]


def _check(name, B, row, placed, after, cap):
    """the oracle's cloud `row` [B] shows what the case is named for"""
    hit = row < 1.0
    assert ((row > 0.0) & (row <= 1.0)).all(), (name, row)
    if name in ("none", "absent", "removed"):
        assert not hit.any(), (name, np.nonzero(hit)[0])
    if name == "removed":
        slot = _slots(cap, 6)[5]
        assert placed["flags"][slot] & abi.F_ALIVE and not (after["flags"][slot] & abi.F_ALIVE), "the step must remove the vehicle"
    if name == "wrap":
        assert hit[0] and hit[B - 1] and hit.sum() < B // 2, (name, np.nonzero(hit)[0])
    if name in ("inside_circle", "long_span"):
        assert hit.sum() > (64 if B == 240 else 6), (name, hit.sum())
    if name == "many":
        assert hit.sum() > (128 if B == 240 else 15), (name, hit.sum())
        assert len(set(np.round(row[hit], 4))) > 3
    if name == "tie":
        assert hit[B // 5], name


def run(cap, B, step_engine=True):
    """-> cases run.  Every case of CASES in one env of one of two rounds, placed into the state the reset left"""
    import oracle_binding as ob
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    cfg = make_config(dict(num_envs=E, num_scenarios=1, map="X", traffic_density=0.0, mover_capacity=cap, auto_reset=False, step_kernel="wg",
                           vehicle_config=dict(lidar=dict(num_lasers=B, distance=50))))
    host = HostScene(cfg)
    L = host.layout
    assert host.cap == cap and host.A == 1 and int(L.n_beams) == B and host.step_kernel == "wg"
    orc = ob.OracleWorld(host)
    eng = None
    if step_engine:
        import torch
        from metadrive_ped_amd.engine import BatchedEngine
        assert torch.cuda.is_available(), "GPU tests need a ROCm device"
        eng = BatchedEngine(cfg, host=host)
        # the lean, non-staged workgroup kernel: narrow at capacity <= 64, its sibling above
        assert eng.k.traffic_mode == 0 and eng.k.agent_idm == 0 and eng.k.num_others == 0 and not eng.k.is_multi_agent
        assert "detected" not in eng.state_dev and eng.w.max_lanes > 64 and eng.cap == cap and eng.k.agents_per_env == 1
        eng.reset()
    orc.reset()
    base = {k: v.copy() for k, v in orc.state.items()}
    keys = ("shape", "dyn", "flags", "nav", "route_roads")
    zero = np.zeros((E, 1, 2), np.float32)
    done = 0
    for r in range(0, len(CASES), E):
        batch = CASES[r:r + E]
        st = orc.state
        for k in keys:
            st[k][...] = base[k]
        for e, (name, make) in enumerate(batch):
            ego = base["shape"][e * cap].copy()
            assert ego["flags"] & abi.F_AGENT
            agent, bodies = make(ego, B, cap)
            for slot, rec in [(0, agent)] + bodies:
                assert 0 <= slot < cap and (slot == 0 or not (base["shape"]["flags"][e * cap + slot] & abi.F_ALIVE)), (name, slot)
                st["shape"][e * cap + slot] = rec
                d = st["dyn"][e * cap + slot]
                d["heading"], d["speed"] = math.atan2(float(rec["s"]), float(rec["c"])), 0.0
                d["last_x"], d["last_y"], d["last_c"], d["last_s"] = rec["cx"], rec["cy"], rec["c"], rec["s"]
                st["dyn"][e * cap + slot] = d
        placed = st["shape"].copy()
        if eng is not None:
            eng.upload_state({k: st[k] for k in keys})
            eng.step(torch.from_numpy(zero).to(eng.device))
        orc.step(zero)
        rows = orc.state["obs"].reshape(E, -1)[:, L.lidar_off:L.lidar_off + B]
        for e, (name, _) in enumerate(batch):
            _check(name, B, rows[e], placed[e * cap:(e + 1) * cap], orc.state["shape"][e * cap:(e + 1) * cap], cap)
            done += 1
        if eng is not None:
            got = eng.download_state()
            where = "cap %d, %d beams, cases %s" % (cap, B, [n for n, _ in batch])
            assert_state_equal(got, orc.state, where=where)
            mine = got["obs"].reshape(E, -1)[:, L.lidar_off:L.lidar_off + B]
            assert np.array_equal(mine.view(np.uint32), rows.view(np.uint32)), where
    return done


@pytest.mark.parametrize("B", [240, 30])
@pytest.mark.parametrize("cap", [24, 72])
def test_md_step_lidar_equals_oracle_on_placed_states(cap, B):
    assert run(cap, B) == len(CASES)

