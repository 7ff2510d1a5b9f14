"""md_flat_cell_item (include/md_geom.h): the lean step kernel's flat pass over the grid cells under the agent's chassis
(contacts_vehicle, kFlat) hands wave lane t item t of the cells' ranges laid end to end.  On the host (tests/contacts_flat_host.c, the
same text the kernel compiles): over seeded random range lengths, walking flat = 0 .. total - 1 visits exactly the (cell, offset)
pairs of the nested loops, in their order; one past the total, and a negative index, answer -1.  Every class of cases is counted."""
import ctypes as C

import numpy as np

import hostlib

ROOM = 400          # pairs per case: above every total used here
MIN_PER_CLASS = 50


def _declare(lib):
    P, i = C.c_void_p, C.c_int
    lib.hx_flat_walk.restype = None
    lib.hx_flat_walk.argtypes = [i, P, i, P, P, P, P]


def _nested(lens):
    """the nested loops of the contacts: cell by cell, offsets ascending"""
    return [(c, o) for c, n in enumerate(lens) for o in range(n)]


def _cases():
    rng = np.random.RandomState(20251020)
    out = []          # (n_cells, four lengths: cells past n_cells hold 0, as the kernel's lanes past n_cells do)

    def add(n_cells, lens):
        lens = list(lens)[:n_cells] + [0] * (4 - n_cells)
        out.append((n_cells, lens))

    for n_cells in (1, 2, 3, 4):
        for _ in range(150):                     # lengths as cells list them: mostly a few dozen items, some none
            add(n_cells, np.where(rng.rand(4) < 0.2, 0, rng.randint(1, 90, 4)))
        for _ in range(60):                      # nothing in any cell
            add(n_cells, [0, 0, 0, 0])
        for z in range(1, 2 ** n_cells):         # zero-length cells in every position, every combination of positions
            for _ in range(6):
                add(n_cells, [0 if (z >> k) & 1 else rng.randint(1, 70) for k in range(4)])
        for total in (1, 63, 64, 65, 127, 128, 129, 200):      # totals on both sides of one and two rounds of 64 lanes, and exactly 64
            for _ in range(12):
                cuts = np.sort(rng.randint(0, total + 1, n_cells - 1))
                add(n_cells, np.diff(np.r_[0, cuts, total]))
    return out


def test_flat_walk_visits_the_nested_loops_pairs_in_their_order():
    cases = _cases()
    lens = np.asarray([l for _, l in cases], np.int32)
    n = len(cases)
    assert lens.min() >= 0 and lens.sum(1).max() < ROOM
    out = np.full((n, ROOM, 2), -7, np.int32)
    pairs, past, before = (np.full(n, -7, np.int32) for _ in range(3))
    p = hostlib.ptr
    hostlib.build("contacts_flat_host", _declare).hx_flat_walk(n, p(lens), ROOM, p(out), p(pairs), p(past), p(before))
    classes = {"n_cells = 1": 0, "n_cells = 2": 0, "n_cells = 3": 0, "n_cells = 4": 0, "total = 0": 0, "total > 64": 0, "total = 64": 0,
               "total > 128": 0, "a zero-length cell before a listed one": 0, "a zero-length last cell": 0}
    for i, (n_cells, l) in enumerate(cases):
        want = _nested(l)
        assert pairs[i] == len(want) == sum(l), (i, l, pairs[i])
        got = [tuple(x) for x in out[i, :pairs[i]].tolist()]
        assert got == want, "case %d lengths %r: flat walk %r..., nested loops %r..." % (i, l, got[:8], want[:8])
        assert (out[i, pairs[i]:] == -7).all()
        assert past[i] == -1 and before[i] == -1, (i, l, past[i], before[i])
        total = sum(l)
        classes["n_cells = %d" % n_cells] += 1
        classes["total = 0"] += total == 0
        classes["total > 64"] += total > 64
        classes["total = 64"] += total == 64
        classes["total > 128"] += total > 128
        classes["a zero-length cell before a listed one"] += any(l[k] == 0 and any(l[k + 1:n_cells]) for k in range(n_cells))
        classes["a zero-length last cell"] += l[n_cells - 1] == 0 and total > 0
    short = {k: v for k, v in classes.items() if v < (12 if k == "total = 64" else MIN_PER_CLASS)}
    assert not short, "classes with too few cases: %r (all: %r)" % (short, classes)
