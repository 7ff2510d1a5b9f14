"""The premise of the road-first localisation (csrc/parts/localize.inc, localize_road_first): the grid cell of a point lists EVERY
lane whose float32 box contains the point, so the lanes of one road taken straight from the lane table are the lanes the
grid walk would have found.  CPU only: the tables of a few small PG maps, the cell computed exactly as the kernel does."""
import numpy as np
import pytest

MAPS = [("straight", "S"), ("curve", "C"), ("ramps", "rR"), ("x_intersection", "X"), ("t_intersection", "T"), ("roundabout", "O")]


def _tables(seq):
    from metadrive_ped_amd.mapgen.pg import PGMap
    from metadrive_ped_amd.mapgen.tables import MapTables
    return MapTables(PGMap(7, lane_num=3, lane_width=3.5, exit_length=50, generate_type="block_sequence", generate_config=seq))


def _cells(mt, x, y):
    """md_floor((x - x0) * inv_cell) in float32, like localize_vehicle; -1 outside the grid"""
    g = mt.grid[0]
    f32 = np.float32
    gx = np.floor((x.astype(f32) - f32(g["x0"])) * f32(g["inv_cell"])).astype(np.int64)
    gy = np.floor((y.astype(f32) - f32(g["y0"])) * f32(g["inv_cell"])).astype(np.int64)
    ok = (gx >= 0) & (gx < g["nx"]) & (gy >= 0) & (gy < g["ny"])
    return np.where(ok, gy * g["nx"] + gx, -1)


@pytest.mark.parametrize("name,seq", MAPS)
def test_cell_lists_every_lane_whose_box_contains_the_point(name, seq):
    mt = _tables(seq)
    L, g = mt.lanes, mt.grid[0]
    assert len(L) > 0 and (L["x1"] >= L["x0"]).all()
    rng = np.random.RandomState(11)
    w, h = g["nx"] / g["inv_cell"], g["ny"] / g["inv_cell"]
    n = 4000
    px = (g["x0"] + rng.uniform(-2.0, w + 2.0, n)).astype(np.float32)     # the grid's extent, and a little beyond it
    py = (g["y0"] + rng.uniform(-2.0, h + 2.0, n)).astype(np.float32)
    # every box's corners and edge midpoints, and their float32 neighbours on both sides
    ex, ey = [], []
    for r in L:
        xs = [r["x0"], r["x1"], np.float32(0.5) * (r["x0"] + r["x1"])]
        ys = [r["y0"], r["y1"], np.float32(0.5) * (r["y0"] + r["y1"])]
        for x in xs:
            for y in ys:
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        ex.append(np.nextafter(np.float32(x), np.float32(dx * np.inf)) if dx else np.float32(x))
                        ey.append(np.nextafter(np.float32(y), np.float32(dy * np.inf)) if dy else np.float32(y))
    px = np.concatenate([px, np.asarray(ex, np.float32)])
    py = np.concatenate([py, np.asarray(ey, np.float32)])
    cell = _cells(mt, px, py)
    inside = ~((px[:, None] < L["x0"][None]) | (px[:, None] > L["x1"][None]) | (py[:, None] < L["y0"][None]) | (py[:, None] > L["y1"][None]))
    assert inside.any(1).sum() > 500, "the points must actually fall into lane boxes"
    missing = []
    for p in np.nonzero(inside.any(1))[0]:
        assert cell[p] >= 0, "%s: point (%r, %r) is inside a lane box but outside the grid" % (name, px[p], py[p])
        items = mt.cell_items[mt.cell_start[cell[p]]:mt.cell_start[cell[p] + 1]]
        lanes_here = set(int(i) for i in items if i >= 0)
        for l in np.nonzero(inside[p])[0]:
            if int(l) not in lanes_here:
                missing.append((float(px[p]), float(py[p]), int(l)))
    assert not missing, "%s: lanes whose box contains the point but which the cell does not list: %s" % (name, missing[:5])


@pytest.mark.parametrize("name,seq", MAPS)
def test_roads_are_contiguous_and_fit_the_window(name, seq):
    """first = lane - idx names the road's first lane, its lanes follow in idx order; no PG road is wider than the window covers"""
    mt = _tables(seq)
    L = mt.lanes
    ids = np.arange(len(L))
    first = ids - L["idx"]
    assert (L["idx"] >= 0).all() and (L["idx"] < L["n_in_road"]).all()
    assert (L["road"][first] == L["road"]).all() and (L["idx"][first] == 0).all()
    assert (first + L["n_in_road"] <= len(L)).all()
    assert (mt.roads["first_lane"][L["road"]] == first).all() and (mt.roads["n_lanes"][L["road"]] == L["n_in_road"]).all()
    assert L["n_in_road"].max() <= 4      # kLocWindow = 3: lanes - 3 .. + 3 hold any road of up to four lanes
