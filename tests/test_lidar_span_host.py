"""md_lidar_beam_span (include/md_geom.h): the cyclic range of beams of a uniform fan whose ray can come within a mover's bounding
radius -- what the lean step kernels' flat lidar pass (lidar_agent_flat) lays over the lanes.  It may only ever be conservative.
On the host (tests/lidar_span_host.c, the same text the kernel compiles, the loops in C): over seeded placements of both shape
families, the ranges and fans of tests/sensor_ref.py and distances from inside the radius to beyond reach, EVERY beam of the fan
is cast with md_ray_shape, built as lidar_item builds it, and every beam with t < 1 must lie inside the span.  Every class of
placements is counted.  The tightness (span length over true hit beams) is printed, not asserted."""
import ctypes as C
import math

import numpy as np
import pytest

import hostlib
import sensor_ref as sr
from metadrive_ped_amd import abi
from metadrive_ped_amd.mapgen.tables import beam_table

PER_COMBO = 9000          # placements per (family, range, fan): 2 x 2 x 6 x 9000 = 216 000
PAD = 0.01                # MD_LIDAR_SPAN_PAD
BOXES = ("vehicle", "barrier", "cyclist", "building")
CIRCLES = ("cone", "warning", "pedestrian")


def _declare(lib):
    P, i = C.c_void_p, C.c_int
    lib.hx_lidar_span.restype = None
    lib.hx_lidar_span.argtypes = [i, P, P, P, P, P, P, P, P, P, P, P]


class Fans:
    """the beam tables of the fans used, laid end to end"""
    def __init__(self, fans):
        self.off, rows, at = {}, [], 0
        for n in fans:
            self.off[n] = at
            rows.append(beam_table(n))
            at += n
        self.table = np.ascontiguousarray(np.concatenate(rows), np.float32)


def run(ego, body, rng, nb, fans):
    n = len(ego)
    ego, body = np.ascontiguousarray(ego), np.ascontiguousarray(body)
    rng = np.ascontiguousarray(rng, np.float32)
    nb = np.ascontiguousarray(nb, np.int32)
    off = np.asarray([fans.off[int(k)] for k in nb], np.int32)
    out = [np.full(n, -7, np.int32) for _ in range(5)]
    p = hostlib.ptr
    hostlib.build("lidar_span_host", _declare).hx_lidar_span(n, p(ego), p(body), p(rng), p(fans.table), p(off), p(nb), *[p(o) for o in out])
    return dict(zip(("first", "count", "hits", "bad", "first_bad"), out))


def radius(body):
    """the unpadded bounding radius, float64"""
    hl, hw = body["hl"].astype(np.float64), body["hw"].astype(np.float64)
    return np.where(sr.is_circle(body["flags"]), hl, np.hypot(hl, hw))


def records(x, y, th, hl, hw, flags):
    r = np.zeros(len(x), abi.SHAPE_DT)
    r["cx"], r["cy"], r["c"], r["s"], r["hl"], r["hw"], r["flags"], r["aux"] = x, y, np.cos(th), np.sin(th), hl, hw, flags, -1
    return r


def placements(draw, names, rng, n):
    """n seeded placements of bodies of the kinds `names` around observers, -> ego, body, the class of every distance"""
    kinds = draw.randint(0, len(names), n)
    hl = np.asarray([sr.BODIES[k][0] for k in names])[kinds] * draw.uniform(0.5, 2.0, n)
    hw = np.asarray([sr.BODIES[k][1] for k in names])[kinds] * draw.uniform(0.5, 2.0, n)
    flags = np.asarray([sr.BODIES[k][2] for k in names])[kinds]
    far = draw.rand(n) < 0.1                                        # a tenth of the observers far from the origin
    ex = draw.uniform(-40.0, 40.0, n) + np.where(far, sr.FAR_ORIGIN[0], 0.0)
    ey = draw.uniform(-40.0, 40.0, n) + np.where(far, sr.FAR_ORIGIN[1], 0.0)
    ego = records(ex, ey, draw.uniform(-math.pi, math.pi, n), 2.25, 0.9, abi.KIND_VEHICLE | abi.F_ALIVE)
    probe = records(ex, ey, np.zeros(n), hl, hw, flags)
    rb = radius(probe)
    cls = draw.choice(5, n, p=(0.15, 0.2, 0.45, 0.1, 0.1))
    u = draw.rand(n)
    dist = np.select([cls == 0, cls == 1, cls == 2, cls == 3, cls == 4],
                     [u * (rb + PAD),                                   # inside the radius
                      rb + PAD + u * 2.0,                               # just outside it: spans of up to half the fan
                      rb + u * rng,                                     # anywhere within reach
                      rng + rb - 0.5 + u * 1.0,                         # around the end of the reach
                      rng + rb + 0.5 + u * 20.0])                       # beyond it
    ang = draw.uniform(-math.pi, math.pi, n)
    body = records(ex + dist * np.cos(ang), ey + dist * np.sin(ang), draw.uniform(-math.pi, math.pi, n), hl, hw, flags)
    return ego, body, cls


def test_every_hit_beam_lies_inside_the_span(capsys):
    fans = Fans(sr.LIDAR_FANS)
    draw = np.random.RandomState(20261021)
    parts = []
    for fam, names in (("box", BOXES), ("circle", CIRCLES)):
        for rng in sr.LIDAR_RANGES:
            for nb in sr.LIDAR_FANS:
                ego, body, cls = placements(draw, names, rng, PER_COMBO)
                parts.append((ego, body, np.full(PER_COMBO, rng, np.float32), np.full(PER_COMBO, nb, np.int32), cls,
                              np.full(PER_COMBO, fam == "box")))
    ego, body, rng, nb, cls, box = (np.concatenate([p[k] for p in parts]) for k in range(6))
    n = len(ego)
    assert n >= 200000
    assert sr.is_circle(body["flags"][~box]).all() and not sr.is_circle(body["flags"][box]).any()
    r = run(ego, body, rng, nb, fans)
    bad = np.nonzero(r["bad"])[0]
    assert not len(bad), "%d of %d placements have a hit beam outside the span; first: case %d fan %d range %g beam %d span (%d, %d) ego %r body %r" % (
        len(bad), n, bad[0], nb[bad[0]], rng[bad[0]], r["first_bad"][bad[0]], r["first"][bad[0]], r["count"][bad[0]], ego[bad[0]], body[bad[0]])
    assert ((r["first"] >= 0) & (r["first"] < nb) & (r["count"] >= 0) & (r["count"] <= nb)).all()
    assert (r["hits"] <= r["count"]).all()
    wrapped = (r["first"] + r["count"] > nb) & (r["count"] < nb)
    classes = {"boxes": int(box.sum()), "circle kinds": int((~box).sum()),
               "inside the radius": int((cls == 0).sum()), "just outside it": int((cls == 1).sum()), "within reach": int((cls == 2).sum()),
               "around the end of the reach": int((cls == 3).sum()), "beyond reach": int((cls == 4).sum()),
               "placements with a hit": int((r["hits"] > 0).sum()), "count = n_beams": int((r["count"] == nb).sum()),
               "count = 0": int((r["count"] == 0).sum()), "spans across beam n - 1 | 0": int(wrapped.sum()),
               "spans longer than 64 beams": int(((r["count"] > 64) & (r["count"] < nb)).sum()),
               "fans below 64 beams": int((nb < 64).sum()), "hits at the end of the reach": int(((cls == 3) & (r["hits"] > 0)).sum())}
    short = {k: v for k, v in classes.items() if v < 1000}
    assert not short, "classes with too few placements: %r (all: %r)" % (short, classes)
    assert (r["count"][cls == 0] == nb[cls == 0]).all()                 # inside the radius: every beam
    beyond = cls == 4                                                   # 0.5 m and more past range + radius: out of reach
    assert (r["count"][beyond] == 0).all() and (r["hits"][beyond] == 0).all()
    hit = (r["hits"] > 0) & (cls != 0)
    with capsys.disabled():
        print("\nmd_lidar_beam_span tightness (span beams / hit beams, placements with a hit, ego outside the radius): all fans %.2f; 240 beams %.2f "
              "(mean span %.1f, mean hit beams %.1f); placements %d, %r" % (
                  r["count"][hit].sum() / r["hits"][hit].sum(), r["count"][hit & (nb == 240)].sum() / r["hits"][hit & (nb == 240)].sum(),
                  r["count"][hit & (nb == 240)].mean(), r["hits"][hit & (nb == 240)].mean(), n, classes))


def _one(ego, b, rng, nb):
    fans = Fans(sorted(set([nb])))
    r = run(np.asarray([ego]), np.asarray([b]), [rng], [nb], fans)
    out = {k: int(v[0]) for k, v in r.items()}
    assert out["bad"] == 0, (out, ego, b)
    return out


EGO = sr.ego_at((3.0, -2.0), 0.4)


def _ahead(kind, dist, beam_angle=0.0, th=None, **kw):
    """a body `dist` metres from EGO's centre in the ego-frame direction beam_angle"""
    a = 0.4 + beam_angle
    return sr.body(kind, (3.0 + dist * math.cos(a), -2.0 + dist * math.sin(a)), a if th is None else th, **kw)


def test_ego_on_the_bounding_circle_gets_every_beam():
    """exactly on the circle of the padded radius (d2 == rb * rb in float32), and on the body's own: count = n_beams; one step out: fewer"""
    ego = sr.ego_at((0.0, 0.0), 0.0)
    for kind, rb in (("cone", np.float32(0.2) + np.float32(0.01)), ("cone", np.float32(0.2)),
                     ("vehicle", np.sqrt(np.float32(2.2) * np.float32(2.2) + np.float32(0.9) * np.float32(0.9), dtype=np.float32) + np.float32(0.01))):
        b = sr.body(kind, (float(rb), 0.0), 0.3)
        assert float(b["cx"]) == float(rb)
        assert _one(ego, b, 50.0, 240)["count"] == 240
    b = sr.body("cone", (float((np.float32(0.2) + np.float32(0.01)) * np.float32(1.000001)), 0.0), 0.3)
    out = _one(ego, b, 50.0, 240)
    assert 110 <= out["count"] <= 121 and out["hits"] > 0, out      # just under half a turn: asin(1 / 1.000001) = pi / 2 - 1.4e-3


def test_span_across_the_wrap_of_the_fan():
    out = _one(EGO, _ahead("vehicle", 12.0, th=0.4 + 0.5 * math.pi), 50.0, 240)
    assert out["first"] > 200 and out["first"] + out["count"] > 240 and 0 < out["hits"] <= out["count"] < 40, out
    out = _one(EGO, _ahead("pedestrian", 30.0), 50.0, 30)
    assert out["count"] == 1 and out["first"] == 0 and out["hits"] == 1, out


def test_count_is_clamped_at_the_fan():
    """beside a building, outside its box and its radius by a hair: the span would be longer than the fan"""
    out = _one(EGO, _ahead("building", 7.09, hl=5.0, hw=5.0), 50.0, 30)
    assert 15 <= out["count"] <= 30 and out["hits"] > 0, out
    out = _one(EGO, _ahead("building", 6.0, hl=5.0, hw=5.0), 50.0, 65)
    assert out["count"] == 65 and out["first"] == 0 and out["hits"] > 0, out


@pytest.mark.parametrize("rng", sr.LIDAR_RANGES)
def test_mover_at_range_plus_radius(rng):
    """a pedestrian whose rim touches the end of the beam: centre at range + radius exactly, and 1 mm nearer / 10 cm farther"""
    r = 0.35
    at = _one(EGO, _ahead("pedestrian", rng + r), rng, 240)
    assert at["count"] >= 1, at
    near = _one(EGO, _ahead("pedestrian", rng + r - 1e-3), rng, 240)
    assert near["hits"] >= 1 and near["count"] >= 1, near
    far = _one(EGO, _ahead("pedestrian", rng + r + 0.1), rng, 240)
    assert far["hits"] == 0, far
    gone = _one(EGO, _ahead("pedestrian", (rng + r + PAD) * 1.0001 + 0.01), rng, 240)
    assert gone["count"] == 0 and gone["hits"] == 0, gone


@pytest.mark.parametrize("nb", [1, 2, 3, 30, 63])
def test_short_fans(nb):
    """fans below one wave's 64 lanes, down to one beam: a body on beam 0, one between two beams, one behind the observer"""
    out = _one(EGO, _ahead("vehicle", 10.0, th=0.4 + 0.5 * math.pi), 50.0, nb)
    assert out["hits"] >= 1 and out["first"] + out["count"] >= 1, out
    out = _one(EGO, _ahead("cone", 20.0, beam_angle=math.pi), 50.0, nb)
    assert out["hits"] == (0 if nb % 2 else 1), out
    if nb == 1:
        assert out["count"] == 0, out
    out = _one(EGO, _ahead("building", 3.0, beam_angle=2.0, hl=5.0, hw=5.0), 50.0, nb)      # the ego inside the box: no hit, every beam
    assert out["count"] == nb and out["hits"] == 0, out
