"""The static tables the contact stage walks (mapgen/tables.py: quads + grid), CPU only:
  (a) every quad is what md_obb_quad is right for: counter-clockwise, convex, no degenerate edge;
  (b) the premise of the device's cull (contacts_vehicle, csrc/parts/contacts.inc: the cells under the chassis AABB + 0.05 m): every quad
      the chassis touches is listed in a cell of that range -- the range restated in float32 exactly as the kernel computes it;
  (c) ref_contacts on placed agents against the float64 reference of tests/contact_ref.py, per flag bit where decided;
  (d) the dense scenario scene whose cells list more than 64 quads (the second trip of the device's 64-strided cell loop), which
      tests/test_gpu_contacts.py runs on the device."""
import math

import numpy as np
import pytest

import contact_ref as cr
import oracle_binding as ob
from metadrive_ped_amd import abi

PG_MAPS = [("straight", "S"), ("curve", "C"), ("ramps", "rR"), ("x_intersection", "X"), ("t_intersection", "T"), ("roundabout", "O"),
           ("tollgate", "S$S"), ("split_merge", "SyY")]
SCENES = [("scenario_%d" % i, i) for i in range(4)]
_CACHE = {}


def _tables(seq):
    """one map's tables: a PG block sequence (as tests/test_grid_covers_boxes.py builds it), or scene i of synthetic_scenarios(4, 900)"""
    if seq not in _CACHE:
        if isinstance(seq, int):
            from metadrive_ped_amd.mapgen.tables import StaticTables
            from metadrive_ped_amd.scenario import make_scenario_config, scene_line_quads, synthetic_scenarios
            if "scenes" not in _CACHE:
                _CACHE["scenes"] = synthetic_scenarios(4, 900)
            region = float(make_scenario_config({})["map_region_size"])
            _CACHE[seq] = StaticTables(*scene_line_quads(_CACHE["scenes"][seq]["map_features"], region))
        else:
            from metadrive_ped_amd.mapgen.pg import PGMap
            from metadrive_ped_amd.mapgen.tables import MapTables
            _CACHE[seq] = MapTables(PGMap(7, lane_num=3, lane_width=3.5, exit_length=50, generate_type="block_sequence", generate_config=seq))
    return _CACHE[seq]


@pytest.mark.parametrize("name,seq", PG_MAPS + SCENES)
def test_quads_are_ccw_convex_and_not_degenerate(name, seq):
    mt = _tables(seq)
    assert mt.quads.dtype == np.float32 and mt.quads.shape[1] == 8 and len(mt.quads) > 100 and len(mt.quad_kind) == len(mt.quads)
    q = mt.quads.astype(np.float64).reshape(-1, 4, 2)
    nxt = np.roll(q, -1, 1)
    area = 0.5 * (q[:, :, 0] * nxt[:, :, 1] - nxt[:, :, 0] * q[:, :, 1]).sum(1)
    assert (area > 0).all(), "%s: quads with non-positive signed area (clockwise): %s" % (name, np.nonzero(area <= 0)[0][:5])
    e = nxt - q
    turn = e[:, :, 0] * np.roll(e, -1, 1)[:, :, 1] - e[:, :, 1] * np.roll(e, -1, 1)[:, :, 0]
    assert (turn > 0).all(), "%s: quads with a turn that is not a left turn: %s" % (name, np.nonzero((turn <= 0).any(1))[0][:5])
    length = np.sqrt((e ** 2).sum(-1))
    assert (length >= 0.05).all(), "%s: quads with an edge shorter than 0.05 m: %s" % (name, np.nonzero((length < 0.05).any(1))[0][:5])
    assert set(np.unique(mt.quad_kind)) <= {abi.Q_LINE_WHITE_CONT, abi.Q_LINE_YELLOW_CONT, abi.Q_LINE_BROKEN, abi.Q_SIDEWALK}


def _touched(mt, sh1, lib):
    """the quads ref_obb_quad (the float32 predicate) hits for one chassis record"""
    a = sh1.ctypes.data
    return [int(q) for q in cr.candidate_quads(mt, sh1) if lib.ref_obb_quad(a, mt.quads[q:q + 1].ctypes.data)]


@pytest.mark.parametrize("name,seq", PG_MAPS + SCENES)
def test_cull_range_lists_every_touched_quad(name, seq):
    mt = _tables(seq)
    lib = ob.load()
    g = mt.grid[0]
    assert abs(1.0 / float(g["inv_cell"]) - 8.0) < 1e-6 and mt.quads.flags["C_CONTIGUOUS"]
    poses, tag = cr.table_poses(mt, np.random.RandomState(31))
    assert len(poses) > 2000 and {"random", "edge", "border"} == set(tag)
    walked, gx0, gx1, gy0, gy1 = cr.cull_range(mt.grid, poses)
    nx = int(g["nx"])
    missing, hits, outside, multi = [], 0, 0, 0
    per_tag = dict.fromkeys(("random", "edge", "border"), 0)
    for p in range(len(poses)):
        sh1 = poses[p:p + 1]
        touched = _touched(mt, sh1, lib)
        if not touched:
            continue
        hits += len(touched)
        per_tag[str(tag[p])] += 1
        outside += int(not walked[p])
        listed = set()
        if walked[p]:
            cells = [gy * nx + gx for gy in range(gy0[p], gy1[p] + 1) for gx in range(gx0[p], gx1[p] + 1)]
            assert cells == cr.walked_cells(mt, sh1)
            multi += len(cells) > 1
            for c in cells:
                listed.update(q for q, _ in cr.cell_quads(mt, c))
        missing += [(p, str(tag[p]), q, poses[p].tolist()) for q in touched if q not in listed]
    # the poses must reach the quads from every pose family, ranges of more than one cell included
    assert hits > 1000 and min(per_tag.values()) > 50 and multi > 100, (name, hits, per_tag, multi)
    assert not missing, "%s: %d touched quads that no cell of the walked range lists (%d poses outside the grid); first (pose, family, " \
        "quad, record): %s" % (name, len(missing), outside, missing[:3])


def _placed_host(seq):
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    host = HostScene(make_config(dict(num_envs=8, num_scenarios=1, map=seq, traffic_density=0.0, auto_reset=False)))
    o = ob.OracleWorld(host)
    o.reset()
    return host, o


def test_oracle_contacts_equal_float64_on_placed_agents():
    reached, absent, cases, undecided = {}, {}, 0, 0
    for name, seq in PG_MAPS:
        host, o = _placed_host(seq)
        E, cap = host.E, host.cap
        mt = host.map_tables[0]
        base = {k: o.state[k].copy() for k in ("shape", "flags")}
        fl0 = base["shape"]["flags"].reshape(E, cap)[:, 0]
        assert (fl0 & abi.F_AGENT).all() and (host.world.arrays["env_map"] == 0).all()
        rng = np.random.RandomState(41)
        poses, tag = cr.table_poses(mt, rng, n_random=160, every=max(25, len(mt.quads) // 12), n_border=80)
        poses = poses[rng.permutation(len(poses))[:(min(len(poses), 320) // E) * E]]
        assert 200 <= len(poses) <= 400
        for r in range(len(poses) // E):
            o.state["shape"][...] = base["shape"]
            o.state["flags"][...] = base["flags"]
            rows = np.arange(E) * cap
            for k in ("cx", "cy", "c", "s"):
                o.state["shape"][k][rows] = poses[k][r * E:(r + 1) * E]
            o.call("ref_contacts")
            for e in range(E):
                want, decided = cr.agent_flags(o.state["shape"][e * cap:(e + 1) * cap], 0, mt.quads, mt.quad_kind)
                got = int(o.state["flags"][e * cap]) & cr.CONTACT_BITS
                assert ((got ^ want) & decided) == 0, "%s pose %s: ref_contacts gives %#x, float64 %#x (decided bits %#x)" % (
                    name, o.state["shape"][e * cap].tolist(), got, want, decided)
                cases += 1
                undecided += decided != cr.CONTACT_BITS
                for bit in (0x10, 0x20, 0x40, 0x80):
                    if decided & bit:
                        reached[bit] = reached.get(bit, 0) + bool(want & bit)
                        absent[bit] = absent.get(bit, 0) + (not want & bit)
    print("placed agents", cases, "undecided", undecided, "reached", reached, "absent", absent)
    assert undecided <= cr.UNDECIDED_CAP * cases, (undecided, cases)
    for bit in (0x10, 0x20, 0x40, 0x80):
        assert reached.get(bit, 0) >= 20 and absent.get(bit, 0) >= 20, (hex(bit), reached, absent)


# ---- (d) the dense scene ----

DENSE_LINES, DENSE_SPACING = 40, 0.3


def dense_scenario(seed=900):
    """A scenario description whose road lines are DENSE_LINES parallel solid white polylines DENSE_SPACING apart, along x through the
    origin (the SDC's first position): its grid cells list far more than 64 quads.  No other track than the SDC's."""
    from metadrive_ped_amd.scenario import synthetic_scenario
    sc = synthetic_scenario(seed, n_vehicles=0, n_parked=0, n_pedestrians=0, n_cones=0)
    feats = {k: f for k, f in sc["map_features"].items() if "LANE" in f["type"]}
    x = np.arange(-30.0, 30.001, 1.5)
    for i in range(DENSE_LINES):
        y = np.full_like(x, DENSE_SPACING * i)
        feats["dense_%02d" % i] = {"type": "ROAD_LINE_SOLID_SINGLE_WHITE", "polyline": np.stack([x, y, np.zeros_like(x)], 1).astype(np.float32)}
    sc["map_features"] = feats
    return sc


def dense_strided_pose(mt, hl=cr.AGENT_HL, hw=cr.AGENT_HW):
    """-> (pose record, the one quad it touches): a chassis at 45 degrees to the lines, one corner of which dips 0.03 m into a piece
    of the LAST line from outside the band, in the middle of the piece"""
    q = len(mt.quads) - 20            # a piece of the last line (40 pieces per line), away from the line's ends
    quad = mt.quads[q].astype(np.float64).reshape(4, 2)
    top = int(np.argmax([(quad[i, 1] + quad[(i + 1) % 4, 1]) for i in range(4)]))      # the edge that faces away from the band
    th = -0.75 * math.pi              # diagonal to the lines: one single corner points into the band
    ctr = cr.approach_edge(quad, top, 0.5, -0.03, th, hl, hw)
    return cr.agent_poses(ctr[None], th, hl, hw), q


def test_dense_scene_fills_a_cell_past_the_wave_width():
    from metadrive_ped_amd.scenario import ScenarioHostScene, make_scenario_config
    cfg = make_scenario_config(dict(num_envs=2, num_scenarios=2))
    host = ScenarioHostScene(cfg, [dense_scenario(), dense_scenario()])
    mt = host.map_tables[0]
    assert len(mt.quads) == DENSE_LINES * 40 and (mt.quad_kind == abi.Q_LINE_WHITE_CONT).all()
    assert np.diff(mt.cell_start).max() > 64
    pose, q = dense_strided_pose(mt)
    lib = ob.load()
    assert _touched(mt, pose, lib) == [q], "the pose must touch one quad only"
    hit, decided = cr.obb_quad(pose, mt.quads[q:q + 1])
    assert hit[0] and decided[0]
    cells = [c for c in cr.walked_cells(mt, pose) if q in dict(cr.cell_quads(mt, c))]
    assert cells and all(dict(cr.cell_quads(mt, c))[q] >= 64 for c in cells), [dict(cr.cell_quads(mt, c))[q] for c in cells]
    # the world tables the device reads hold the same lists
    a = host.world.arrays
    assert np.array_equal(a["quads"][:len(mt.quads)], mt.quads) and np.array_equal(a["cell_items"][:len(mt.cell_items)], mt.cell_items)
